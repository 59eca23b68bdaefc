#!/usr/bin/env python3
"""One F16Batch.rollout_vjp launch (the rollout's vector-Jacobian product, H reverse steps fused) against the route the package offered
before it, in the same process on the same library: F16Batch.linearize at the H x n flown points (192 floats per point to HBM) followed by
the H-step adjoint recursion in torch — in one linearize launch where the H x n Jacobians fit in `--fit-gb`, chunked step by step where
they do not.  The forward F16Batch.rollout(record_every=1) is timed on its own: the backward-to-forward ratio.

    python tools/microbench/rollout_vjp_cost.py [--out profiles/rollout_vjp_cost.json] [--horizon 50]

The phase split: build np_model_rollout_vjp.hip with -DNPF16_VJP_ONLY_PHASE=1 (and 2) into a library of its own and run
`NPF16_LIB=that.so ... --only-vjp --sizes 65536,1000000`: the kernel with the other phase's arithmetic left out (loop, barriers, loads kept).

Timing: HIP events around each variant on the current stream, after warm-up calls of every variant; the variants alternate inside every
repeat; the median of the repeats is reported with min / max (tools/microbench/linearize_cost.py::timed).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from linearize_cost import timed  # noqa: E402

SIZES = [3_000, 65_536, 1_000_000]
DT, LAG_KEEP = 0.02, 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--horizon', type=int, default=50)
    ap.add_argument('--fit-gb', type=float, default=16.0)
    ap.add_argument('--sizes', default=','.join(map(str, SIZES)))
    ap.add_argument('--only-vjp', action='store_true', help='time rollout_vjp alone (measurement builds of the kernel)')
    args = ap.parse_args()
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    H, cases = args.horizon, []
    gain = torch.tensor([0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5], device='cuda').view(4, 1)
    for n in map(int, args.sizes.split(',')):
        warmup, repeats = (3, 15) if n <= 100_000 else (1, 5)
        b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=1)
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(n)
        act = (torch.rand((H, n, 4), device='cuda', generator=g) * 2 - 1) * 0.6
        s0, u0 = b.s.clone(), b.u.clone()
        traj = b.rollout(act, s0, u0, record_every=1)[2]
        G, gu = torch.randn((H, 12, n), device='cuda', generator=g), torch.randn((5, n), device='cuda', generator=g)
        one_launch = H * n * 192 * 4 <= args.fit_gb * 2 ** 30

        def linearize_then_torch():
            u, us = u0[:4], []
            for t in range(H):   # the lag, forward
                u = LAG_KEEP * u + gain * act[t].clamp(-1, 1).t()
                us.append(torch.cat((u, u0[4:])))
            pts = torch.cat((s0[None], traj[:-1]))
            if one_launch:
                _, A, B = b.linearize(pts.permute(1, 0, 2).reshape(12, H * n), torch.stack(us, 1).reshape(5, H * n), want_xdot=False)
                A, B = A.view(12, 12, H, n), B.view(12, 4, H, n)
            ls, lu, ga = torch.zeros_like(s0), gu[:4], [None] * H
            for t in reversed(range(H)):
                At, Bt = (A[:, :, t], B[:, :, t]) if one_launch else b.linearize(pts[t], us[t], want_xdot=False)[1:]
                ls = G[t] + ls
                mu = lu + DT * (ls[:, None] * Bt).sum(0)
                ga[t] = torch.where(act[t].t().abs() <= 1, gain * mu, torch.zeros_like(mu))
                lu, ls = LAG_KEEP * mu, ls + DT * (ls[:, None] * At).sum(0)
            return ls, lu, ga

        fns = {'rollout_vjp': lambda: b.rollout_vjp(act, traj, G, gu, s=s0, u=u0), 'rollout_forward': lambda: b.rollout(act, s0, u0, record_every=1),
               'linearize_then_torch': linearize_then_torch}
        rec = {'n': n, 'horizon': H, 'baseline_one_linearize_launch': one_launch, 'library': os.environ.get('NPF16_LIB', 'built')}
        if args.only_vjp:
            rec.update(timed({'rollout_vjp': fns['rollout_vjp']}, warmup, repeats))
            rec['vjp_ms_per_step'] = rec['rollout_vjp']['median_ms'] / H
            cases.append(rec)
            print(json.dumps(rec), flush=True)
            continue
        rec.update(timed(fns, warmup, repeats))
        rec['vjp_ms_per_step'] = rec['rollout_vjp']['median_ms'] / H
        rec['backward_over_forward'] = rec['rollout_vjp']['median_ms'] / rec['rollout_forward']['median_ms']
        rec['baseline_over_vjp'] = rec['linearize_then_torch']['median_ms'] / rec['rollout_vjp']['median_ms']
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        del b, act, traj, G
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/rollout_vjp_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
