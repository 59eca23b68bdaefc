#!/usr/bin/env python3
"""One F16Batch.trim call against the route the package offered before, in the same process on the same library: the loop of
examples/trim_linearize.py — per Newton step one F16Batch.linearize launch (all 192 planes of [xdot | A | B] to HBM), the selection of J
and r in torch and a torch.linalg.solve — for as many steps as the call's slowest row took (the loop has no per-row exit, no line search,
no bounds and no status).  Both routes start from the same flight conditions and are timed the same way.

    python tools/microbench/trim_cost.py [--out profiles/trim_cost.json]

Timing: HIP events around each route on the current stream, after warm-up calls of both; the routes alternate inside every repeat; the
median of the repeats is reported with min / max.  Also recorded: the mean and the largest iters of the call, its statuses, and the share
of rows and of 64-row tiles that ran a backtracking pass (the call's optional per-row count of refused full steps).
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tools.microbench.linearize_cost import timed  # noqa: E402

SIZES = [3_000, 65_536, 1_000_000]


def flight_conditions(kind, n):
    """level and climbing flight over 5 000-25 000 ft and 400-800 ft/s, turns of +-3 deg/s: s [12, n], u [5, n], target [12, n]"""
    k = torch.arange(n, device='cuda', dtype=torch.float32)
    s, u, tgt = torch.zeros((12, n), device='cuda'), torch.zeros((5, n), device='cuda'), torch.zeros((12, n), device='cuda')
    s[2], s[6] = 5000 + 20000 * ((k * 37) % n) / max(n - 1, 1), 400 + 400 * k / max(n - 1, 1)
    gamma = torch.where(k % 2 == 1, 0.05, 0.0)
    s[7], s[4], u[0] = 0.05, 0.05 + gamma, 3000.0
    if kind == 'turn':
        tgt[2], tgt[5] = s[6] * torch.sin(gamma), torch.where(k % 4 < 2, 1.0, -1.0) * math.radians(3.0)
        s[3] = torch.atan(tgt[5] * s[6] / 32.17)
    return s, u, tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from neuralplane_amd import _lib
    from neuralplane_amd.core import F16Batch, trim_problem
    from neuralplane_amd.envs.utils.utils import parse_config
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = F16Batch(8, parse_config('heading'), 'heading', 'cuda:0', seed=1)
    cases = []
    for kind in ('longitudinal', 'turn'):
        D, rows, scale, lo, hi = trim_problem(kind)
        Dd, sc = D.cuda(), torch.tensor(scale, device='cuda')[rows]
        for n in SIZES:
            warmup, repeats = (3, 20) if n <= 100_000 else (2, 7)
            s0, u0, tgt = flight_conditions(kind, n)
            bt = torch.zeros(n, dtype=torch.int32, device='cuda')
            out = b.trim(s0, u0, D, rows, target=tgt, scale=scale, lo=lo, hi=hi, backtracks=bt)
            tiles = torch.nn.functional.pad(bt, (0, -n % 64)).view(-1, 64)   # a tile runs value passes when one of its rows backtracks
            iters, status = out[3], out[4]
            steps = int(iters.max().item())

            def torch_loop():
                z = torch.cat([s0, u0[:4]]).clone()
                for _ in range(steps + 1):
                    xdot, A, B = b.linearize(z[:12], torch.cat([z[12:], u0[4:]]))
                    J = torch.einsum('ken,ej->nkj', torch.cat([A, B], 1)[rows], Dd) / sc[None, :, None]
                    r = ((xdot - tgt)[rows] / sc[:, None]).t()
                    z += Dd @ torch.linalg.solve(J, -r).t()
                return z

            fns = {'trim': lambda: b.trim(s0, u0, D, rows, target=tgt, scale=scale, lo=lo, hi=hi), 'linearize_loop': torch_loop}
            rec = {'kind': kind, 'm': len(rows), 'n': n, 'num_cus': cus, 'groups': _lib.linearize_groups(n, cus), 'linearize_loop_launches': steps + 1,
                   'iters_mean': float(iters.float().mean().item()), 'iters_max': steps,
                   'rows_that_backtracked': float((bt > 0).float().mean().item()), 'tiles_that_backtracked': float((tiles > 0).any(1).float().mean().item()),
                   'status_counts': {str(k): int((status == k).sum().item()) for k in range(5)}}
            rec.update(timed(fns, warmup, repeats))
            rec['linearize_loop_over_trim'] = rec['linearize_loop']['median_ms'] / rec['trim']['median_ms']
            cases.append(rec)
            print(json.dumps(rec), flush=True)
            del s0, u0, tgt, out
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/trim_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
