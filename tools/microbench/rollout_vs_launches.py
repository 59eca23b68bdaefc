#!/usr/bin/env python3
"""H = 50 look-ahead steps through F16Batch.rollout (ONE launch) against the same 50 steps as F16Batch.update launches (what the
package offered before), in one process on one library.  The baseline is always the launch loop, never the new kernel against itself.

    python tools/microbench/rollout_vs_launches.py [--out profiles/rollout_vs_launches.json] [--shapes]

Timing: HIP events around the whole H-step window on the current stream, after warm-up windows of every variant; the variants alternate
inside every repeat; the median of the repeats is reported with min / max.  --shapes also times both pinned shapes of the rollout kernel (the sweep behind the shape rule's threshold).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
H = 50
CASES = [(3_000, 1), (10_000, 1), (65_536, 1), (1_000_000, 1), (1_000, 64)]   # (n0, fanout)
SHAPE_SWEEP = [(16_384, 1), (24_576, 1), (32_768, 1)]                      # --shapes: more sizes around the shape rule's threshold


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
    ap.add_argument('--shapes', action='store_true')
    ap.add_argument('--solver', default=None)
    args = ap.parse_args()
    from neuralplane_amd import _lib
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_out = []
    for n0, fanout in sorted(CASES + (SHAPE_SWEEP if args.shapes else []), key=lambda c: (c[1], c[0])):
        rows = n0 * fanout
        warmup, repeats = (3, 20) if rows <= 100_000 else (2, 7)
        b = F16Batch(n0, parse_config('heading'), 'heading', 'cuda:0', seed=1, solver=args.solver)
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(n0)
        a = (torch.rand((H, rows, 4), device='cuda', generator=g) * 2 - 1) * 0.3
        # the launch loop advances a batch of `rows` aircraft: with a fan-out that is K copies of the state made in torch first
        loop = b if fanout == 1 else F16Batch(rows, parse_config('heading'), 'heading', 'cuda:0', seed=1, solver=args.solver)
        src = torch.arange(rows, device='cuda') // fanout
        s0, u0 = b.s.clone(), b.u.clone()

        def launches():
            loop.s.copy_(s0[:, src] if fanout > 1 else s0)      # restore (clone-and-restore is part of a look-ahead on this path)
            loop.u.copy_(u0[:, src] if fanout > 1 else u0)
            for t in range(H):
                loop.update(a[t])

        fns = {'update_launches': launches, 'rollout': lambda: b.rollout(a, s=s0, u=u0, fanout=fanout)}
        if args.shapes:
            fns['rollout_throughput'] = lambda: b.rollout(a, s=s0, u=u0, fanout=fanout, shape='throughput')
            if args.solver != 'rk4' and rows <= 200_000:
                fns['rollout_split'] = lambda: b.rollout(a, s=s0, u=u0, fanout=fanout, shape='split')
        rec = {'n0': n0, 'fanout': fanout, 'rows': rows, 'horizon': H, 'solver': args.solver or 'euler', 'num_cus': cus,
               'auto_shape': _lib.rollout_shape(rows, cus, 1 if args.solver == 'rk4' else 0)}
        rec.update(timed(fns, warmup, repeats))
        end = b.rollout(a, s=s0, u=u0, fanout=fanout)
        launches()
        rec['bit_identical'] = bool(torch.equal(end[0], loop.s) and torch.equal(end[1], loop.u))
        rec['speedup'] = rec['update_launches']['median_ms'] / rec['rollout']['median_ms']
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)
        del b, loop
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/rollout_vs_launches.py', 'device': torch.cuda.get_device_name(0), 'cases': rows_out}, f, indent=1)


if __name__ == '__main__':
    main()
