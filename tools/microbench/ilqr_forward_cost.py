#!/usr/bin/env python3
"""One F16Batch.ilqr_forward launch (iLQR's forward pass: H steps under the feedback law, L step sizes per problem) against the route it
replaces — H F16Batch.update launches on the P * L rows with the 4 x 16 mat-vec in torch between them — and against the open-loop
F16Batch.rollout(record_every=1) of the same rows (the price of the feedback).  HIP-event medians, one process.

    python tools/microbench/ilqr_forward_cost.py [--out profiles/ilqr_forward_cost.json] [--horizon 50] [--cases 375x8,8192x8,125000x8,65536x1]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from linearize_cost import timed  # noqa: E402

LAG_KEEP = 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--horizon', type=int, default=50)
    ap.add_argument('--cases', default='375x8,8192x8,125000x8,65536x1', help='PxL, comma separated')
    args = ap.parse_args()
    from neuralplane_amd import _lib
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    H, cases = args.horizon, []
    gain = torch.tensor([0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5], device='cuda')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for P, L in (tuple(map(int, c.split('x'))) for c in args.cases.split(',')):
        rows = P * L
        warmup, repeats = (3, 15) if rows <= 100_000 else (1, 5)
        b = F16Batch(rows, parse_config('heading'), 'heading', 'cuda:0', seed=1)   # rows aircraft: the launch loop steps them in place
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(rows)
        act = (torch.rand((H, P, 4), device='cuda', generator=g) * 2 - 1) * 0.6
        s0, u0 = b.s[:, :P].clone(), b.u[:, :P].clone()
        traj = b.rollout(act, s0, u0, record_every=1)[2]
        # gains of a plausible size: the timing does not depend on their values, only on finite flights
        k, K = 1e-2 * torch.randn((H, 4, P), device='cuda', generator=g), 1e-4 * torch.randn((H, 4, 16, P), device='cuda', generator=g)
        alphas = [2.0 ** -i for i in range(L)]
        hs, ha = torch.rand((H, 12), generator=torch.Generator().manual_seed(rows)) * 1e-2, torch.ones(4)
        alpha_rows = torch.tensor(alphas, device='cuda').repeat(P)
        rep = lambda x: x.repeat_interleave(L, -1)  # noqa: E731

        def launch_loop():   # the route before this call: per step one mat-vec in torch on the P * L rows, then one update launch
            b.s.copy_(rep(s0))
            b.u.copy_(rep(u0))
            ub, acts, states = u0[:4], [], []
            for t in range(H):
                xb = torch.cat((s0 if t == 0 else traj[t - 1], ub))
                d = torch.cat((b.s, b.u[:4])) - rep(xb)
                a = rep(act[t].t()) + alpha_rows * rep(k[t]) + torch.einsum('ajp,jp->ap', rep(K[t]), d)
                a = a.clamp(-1, 1).t().contiguous()
                b.update(a)
                acts.append(a)
                states.append(b.s.clone())
                ub = LAG_KEEP * ub + gain[:, None] * act[t].clamp(-1, 1).t()
            return acts, states

        act_rows = rep(act.transpose(1, 2)).transpose(1, 2).contiguous()
        fns = {'ilqr_forward': lambda: b.ilqr_forward(act, traj, k, K, alphas, s=s0, u=u0),
               'ilqr_forward_with_cost': lambda: b.ilqr_forward(act, traj, k, K, alphas, s=s0, u=u0, cost=(hs, ha, traj)),
               'rollout_open_loop': lambda: b.rollout(act_rows, s0, u0, fanout=L, record_every=1),
               'update_launch_loop': launch_loop}
        rec = {'problems': P, 'n_alpha': L, 'rows': rows, 'horizon': H, 'shape': _lib.rollout_shape(rows, cus)}
        rec.update(timed(fns, warmup, repeats))
        rec['loop_over_forward'] = rec['update_launch_loop']['median_ms'] / rec['ilqr_forward']['median_ms']
        rec['forward_over_open_loop'] = rec['ilqr_forward']['median_ms'] / rec['rollout_open_loop']['median_ms']
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        del b, act, traj, k, K, act_rows
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/ilqr_forward_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
