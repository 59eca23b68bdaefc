#!/usr/bin/env python3
"""One F16Batch.ekf launch (H predict + update steps fused) against the route the package offered before it — per step F16Batch.linearize,
F16Batch.rollout(horizon=1), two torch.bmm and a torch.linalg.solve — and against F16Batch.ilqr_backward, which runs the same tile plus an
MFMA phase.  HIP-event medians of 7, one process, warm clocks.

    python tools/microbench/ekf_cost.py [--out profiles/ekf_cost.json] [--horizon 50] [--only-ekf]

The phase split: build np_model_ekf.hip with -DNPF16_EKF_ONLY_PHASE=12 (phase 3 left out) into a library of its own and run
NPF16_LIB=<that library> python tools/microbench/ekf_cost.py --only-ekf.
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
SENSORS = [2, 3, 4, 5, 6, 9, 10, 11]
SIGMA = [10, 10, 100, 0.01, 0.01, 0.01, 1, 0.001, 0.001, 0.01, 0.01, 0.01, 100, 0.1, 0.1, 0.1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--horizon', type=int, default=50)
    ap.add_argument('--sizes', default=','.join(map(str, SIZES)))
    ap.add_argument('--only-ekf', action='store_true', help='time ekf alone (measurement builds of the kernel)')
    args = ap.parse_args()
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    H, cases, measure = args.horizon, [], sum(1 << k for k in SENSORS)
    sig = torch.tensor(SIGMA, device='cuda')
    S = torch.cat((torch.ones(12, device='cuda'), LAG_KEEP * torch.ones(4, device='cuda')))
    q, r = ((0.05 * sig) ** 2).tolist(), ((0.5 * sig) ** 2).tolist()
    nvec = torch.zeros(16, device='cuda')
    nvec[SENSORS] = 1 / torch.tensor(r, device='cuda')[SENSORS]
    eye16 = torch.eye(16, device='cuda')
    for n in map(int, args.sizes.split(',')):
        b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=1)
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(n)
        act = (torch.rand((H, n, 4), device='cuda', generator=g) * 2 - 1) * 0.6
        s0, u0 = b.s.clone(), b.u.clone()
        traj = b.rollout(act, s0, u0, record_every=1)[2]
        z = torch.zeros((H, 16, n), device='cuda')
        z[:, :12] = traj + 0.5 * sig[:12, None] * torch.randn((H, 12, n), device='cuda', generator=g)
        P0 = torch.diag(sig ** 2)[:, :, None].repeat(1, 1, n)

        def torch_route():
            s, u, P = s0, u0, P0.permute(2, 0, 1)
            for t in range(H):
                s1, u1 = b.rollout(act[t:t + 1], s, u)
                _, A, B = b.linearize(s, u1, want_xdot=False)
                F = eye16.repeat(n, 1, 1)
                F[:, :12] += DT * torch.cat((A, B), 1).permute(2, 0, 1)
                F = F * S
                Pm = torch.bmm(F, torch.bmm(P, F.transpose(1, 2)))
                Pm = 0.5 * (Pm + Pm.transpose(1, 2)) + torch.diag(torch.tensor(q, device='cuda'))
                xm = torch.cat((s1, u1[:4])).t()
                P = torch.linalg.solve(eye16 + Pm * nvec, Pm)
                P = 0.5 * (P + P.transpose(1, 2))
                x = xm + torch.bmm(P, (nvec * (z[t].t() - xm))[:, :, None])[:, :, 0]
                s, u = x[:, :12].t().contiguous(), torch.cat((x[:, 12:].t(), u1[4:]))
            return s, u, P

        fns = {'ekf': lambda: b.ekf(act, z, P0, q, r, measure, s=s0, u=u0)}
        if not args.only_ekf:
            G, ga = torch.randn((H, 12, n), device='cuda', generator=g), torch.randn((H, 4, n), device='cuda', generator=g)
            hs, ha = torch.rand((H, 12), generator=torch.Generator().manual_seed(n)) * 1e-2, torch.ones(4)
            fns['ilqr_backward'] = lambda: b.ilqr_backward(act, traj, G, ga, hs, ha, 1e-3, s=s0, u=u0)
            fns['torch_route'] = torch_route
        rec = {'n': n, 'horizon': H, 'sensors': len(SENSORS), 'library': os.environ.get('NPF16_LIB', 'built')}
        rec.update(timed(fns, 2, 7))
        rec['ekf_ms_per_step'] = rec['ekf']['median_ms'] / H
        if not args.only_ekf:
            rec['ekf_over_ilqr_backward'] = rec['ekf']['median_ms'] / rec['ilqr_backward']['median_ms']
            rec['torch_route_over_ekf'] = rec['torch_route']['median_ms'] / rec['ekf']['median_ms']
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        del b, act, traj, z, P0
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/ekf_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
