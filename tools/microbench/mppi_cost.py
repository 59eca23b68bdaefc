#!/usr/bin/env python3
"""One F16Batch.mppi call (an MPPI iteration: sample, fly, cost, re-weight; two launches) against the open-loop F16Batch.rollout of the same
rows (the price of noise plus cost) and against the route it replaces: examples/lookahead_mppi.py's torch sequence around
rollout(record_every=1) with the same cost, its K-fold copies counted.  HIP-event medians, one process.  The share
of the re-weighting kernel comes from a profiler pass of its own, after the timing.

    python tools/microbench/mppi_cost.py [--out profiles/mppi_cost.json] [--horizon 50] [--cases 47x64,1024x64,15625x64,64x1024]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from linearize_cost import timed  # noqa: E402

SIGMA, TEMPERATURE = 0.2, 0.5


def kernel_share(fn, calls=5):
    """(update kernel's device time, rollout kernel's) per call in ms from the profiler's kernel records, or None if it records none"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    us = {'update': 0.0, 'rollout': 0.0}
    for ev in prof.events():
        for k in us:
            if f'f16_mppi_{k}_kernel' in ev.name:
                us[k] += getattr(ev, 'device_time', None) or getattr(ev, 'cuda_time', 0.0)
    return None if not us['rollout'] else {k: v / calls / 1e3 for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--horizon', type=int, default=50)
    ap.add_argument('--cases', default='47x64,1024x64,15625x64,64x1024', help='PxK, comma separated')
    args = ap.parse_args()
    from neuralplane_amd import _lib
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    H, cases = args.horizon, []
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for P, K in (tuple(map(int, c.split('x'))) for c in args.cases.split(',')):
        rows = P * K
        warmup, repeats = (3, 15) if rows <= 100_000 else (1, 5)
        b = F16Batch(P, parse_config('heading'), 'heading', 'cuda:0', seed=1)
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(rows)
        act = (torch.rand((H, P, 4), device='cuda', generator=g) * 2 - 1) * 0.6
        s0, u0 = b.s.clone(), b.u.clone()
        s_ref = b.rollout(act, s0, u0, record_every=1)[2]
        hs, ha = torch.rand((H, 12), generator=torch.Generator().manual_seed(rows)) * 1e-2, torch.ones(4)
        hs_d, ha_d = hs.cuda(), ha.cuda()
        act_rows = act.repeat_interleave(K, dim=1)

        def torch_route():   # what a user writes around the one fused rollout call: noise, K copies of the plan, the trajectory read back
            noise = SIGMA * torch.randn((H, rows, 4), device='cuda', generator=g)
            cand = (act.repeat_interleave(K, dim=1) + noise).clamp(-1, 1)
            traj = b.rollout(cand, s0, u0, fanout=K, record_every=1)[2]
            e = traj - s_ref.repeat_interleave(K, 2)
            cost = 0.5 * (hs_d[:, :, None] * e ** 2).sum((0, 1)) + 0.5 * (ha_d * cand ** 2).sum((0, 2))
            c = torch.nan_to_num(cost, nan=1e6, posinf=1e6).view(P, K)
            w = torch.softmax(-(c - c.min(1, keepdim=True).values) / TEMPERATURE, dim=1)
            return (w.t().reshape(1, K, P, 1) * cand.view(H, P, K, 4).transpose(1, 2)).sum(1)

        mppi = lambda: b.mppi(act, SIGMA, TEMPERATURE, cost=(hs, ha, s_ref), candidates=K, s=s0, u=u0)  # noqa: E731
        fns = {'mppi': mppi, 'rollout_open_loop': lambda: b.rollout(act_rows, s0, u0, fanout=K), 'torch_route': torch_route}
        rec = {'problems': P, 'candidates': K, 'rows': rows, 'horizon': H, 'shape': _lib.rollout_shape(rows, cus)}
        rec.update(timed(fns, warmup, repeats))
        rec['torch_route_over_mppi'] = rec['torch_route']['median_ms'] / rec['mppi']['median_ms']
        rec['mppi_over_open_loop'] = rec['mppi']['median_ms'] / rec['rollout_open_loop']['median_ms']
        rec['kernel_ms'] = kernel_share(mppi)
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        del b, act, s_ref, act_rows
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/mppi_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
