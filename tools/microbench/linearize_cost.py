#!/usr/bin/env python3
"""One F16Batch.linearize launch (xdot, A, B per row) against two baselines in the same process on the same library: one F16Batch.update
launch (one model evaluation per row), and the finite-difference route the package offered before — F16Batch.rollout(fanout=28, horizon=1),
i.e. 28 model evaluations per row (central differences in 14 directions), plus the differencing in torch.  The finite-difference figure is a
lower bound of that route's cost: building the 28 perturbed flight conditions per row is not counted.

    python tools/microbench/linearize_cost.py [--out profiles/linearize_cost.json]

Timing: HIP events around each variant on the current stream, after warm-up calls of every variant; the variants alternate inside every
repeat; the median of the repeats is reported with min / max.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
SIZES = [3_000, 65_536, 1_000_000]
FD_EVALS = 28


def timed(fns, warmup, repeats):
    """{name: fn} -> {name: stats}; the variants alternate inside every repeat, so drift of the shared machine hits all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'repeats': repeats} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from neuralplane_amd import _lib
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = []
    for n in SIZES:
        warmup, repeats = (3, 20) if n <= 100_000 else (2, 7)
        b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=1)
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(n)
        a1 = (torch.rand((n, 4), device='cuda', generator=g) * 2 - 1) * 0.3
        a28 = (torch.rand((n * FD_EVALS, 4), device='cuda', generator=g) * 2 - 1) * 0.3
        s0, u0 = b.s.clone(), b.u.clone()
        stepper = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=1)
        stepper.reset(want_obs=False)

        def finite_differences():
            s_end, _ = b.rollout(a28, s=s0, u=u0, fanout=FD_EVALS, horizon=1)
            pair = s_end.view(12, n, FD_EVALS // 2, 2)
            return (pair[..., 1] - pair[..., 0]) * 0.5e3

        fns = {'linearize': lambda: b.linearize(s0, u0), 'update': lambda: stepper.update(a1), 'finite_differences': finite_differences}
        rec = {'n': n, 'num_cus': cus, 'groups': _lib.linearize_groups(n, cus), 'fd_evaluations_per_row': FD_EVALS}
        rec.update(timed(fns, warmup, repeats))
        rec['linearize_over_update'] = rec['linearize']['median_ms'] / rec['update']['median_ms']
        rec['finite_differences_over_linearize'] = rec['finite_differences']['median_ms'] / rec['linearize']['median_ms']
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        del b, stepper, a28
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/linearize_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
