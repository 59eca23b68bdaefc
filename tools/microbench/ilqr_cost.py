#!/usr/bin/env python3
"""One F16Batch.ilqr_backward launch (iLQR's Riccati sweep, H steps fused) against the route the package offered before it — F16Batch.linearize
at the flown points, then the same recursion with torch.bmm / torch.linalg.cholesky_ex — and against F16Batch.rollout_vjp, whose tile it
extends.  HIP-event medians, one process.

    python tools/microbench/ilqr_cost.py [--out profiles/ilqr_cost.json] [--horizon 50] [--only-ilqr]

The phase split: build np_model_ilqr.hip with -DNPF16_ILQR_ONLY_PHASE=12 (phase 3 left out) into a library of its own and run
NPF16_LIB=<that library> python tools/microbench/ilqr_cost.py --only-ilqr.
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
DT, LAG_KEEP, MU = 0.02, 0.9, 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--horizon', type=int, default=50)
    ap.add_argument('--fit-gb', type=float, default=16.0)
    ap.add_argument('--sizes', default=','.join(map(str, SIZES)))
    ap.add_argument('--only-ilqr', action='store_true', help='time ilqr_backward alone (measurement builds of the kernel)')
    args = ap.parse_args()
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    H, cases = args.horizon, []
    gain = torch.tensor([0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5], device='cuda')
    S = torch.cat((torch.ones(12, device='cuda'), LAG_KEEP * torch.ones(4, device='cuda')))
    eye4, eye16 = torch.eye(4, device='cuda'), torch.eye(16, device='cuda')
    for n in map(int, args.sizes.split(',')):
        warmup, repeats = (3, 15) if n <= 100_000 else (1, 5)
        b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=1)
        b.reset(want_obs=False)
        g = torch.Generator(device='cuda').manual_seed(n)
        act = (torch.rand((H, n, 4), device='cuda', generator=g) * 2 - 1) * 0.6
        s0, u0 = b.s.clone(), b.u.clone()
        traj = b.rollout(act, s0, u0, record_every=1)[2]
        G, ga, gu = (torch.randn(shape, device='cuda', generator=g) for shape in ((H, 12, n), (H, 4, n), (5, n)))
        hs, ha = torch.rand((H, 12), generator=torch.Generator().manual_seed(n)) * 1e-2, torch.ones(4)
        one_launch = H * n * 192 * 4 <= args.fit_gb * 2 ** 30

        def linearize_then_torch():
            u, us = u0[:4], []
            for t in range(H):   # the lag, forward
                u = LAG_KEEP * u + gain[:, None] * act[t].clamp(-1, 1).t()
                us.append(torch.cat((u, u0[4:])))
            pts = torch.cat((s0[None], traj[:-1]))
            if one_launch:
                _, A, B = b.linearize(pts.permute(1, 0, 2).reshape(12, H * n), torch.stack(us, 1).reshape(5, H * n), want_xdot=False)
                A, B = A.view(12, 12, H, n), B.view(12, 4, H, n)
            p, P = torch.cat((torch.zeros((n, 12), device='cuda'), gu[:4].t()), 1), torch.zeros((n, 16, 16), device='cuda')
            hsd, had, ks, Ks = hs.cuda(), torch.diag_embed(ha.cuda()), [None] * H, [None] * H
            for t in reversed(range(H)):
                At, Bt = (A[:, :, t], B[:, :, t]) if one_launch else b.linearize(pts[t], us[t], want_xdot=False)[1:]
                F = eye16.repeat(n, 1, 1)
                F[:, :12] += DT * torch.cat((At, Bt), 1).permute(2, 0, 1)
                p[:, :12] += G[t].t()
                P.diagonal(dim1=1, dim2=2)[:, :12].add_(hsd[t])
                D = torch.where(act[t].abs() <= 1, gain, torch.zeros((), device='cuda'))
                w, W = torch.bmm(F.transpose(1, 2), p[:, :, None])[:, :, 0], torch.bmm(F.transpose(1, 2), torch.bmm(P, F))
                Qa, Qax = D * w[:, 12:] + ga[t].t(), D[:, :, None] * W[:, 12:] * S
                Qaa = D[:, :, None] * W[:, 12:, 12:] * D[:, None] + had
                L = torch.linalg.cholesky_ex(Qaa + MU * eye4).L
                kt, Kt = -torch.cholesky_solve(Qa[:, :, None], L)[:, :, 0], -torch.cholesky_solve(Qax, L)
                KT = Kt.transpose(1, 2)
                p = S * w + torch.bmm(KT, (torch.bmm(Qaa, kt[:, :, None]) + Qa[:, :, None]))[:, :, 0] + torch.bmm(Qax.transpose(1, 2), kt[:, :, None])[:, :, 0]
                P = S[:, None] * W * S + torch.bmm(KT, torch.bmm(Qaa, Kt) + Qax) + torch.bmm(Qax.transpose(1, 2), Kt)
                P = 0.5 * (P + P.transpose(1, 2))
                ks[t], Ks[t] = kt, Kt
            return ks, Ks

        fns = {'ilqr_backward': lambda: b.ilqr_backward(act, traj, G, ga, hs, ha, MU, g_u_end=gu[:4], s=s0, u=u0),
               'rollout_vjp': lambda: b.rollout_vjp(act, traj, G, gu, s=s0, u=u0), 'linearize_then_torch': linearize_then_torch}
        rec = {'n': n, 'horizon': H, 'baseline_one_linearize_launch': one_launch, 'library': os.environ.get('NPF16_LIB', 'built')}
        rec.update(timed({'ilqr_backward': fns['ilqr_backward']} if args.only_ilqr else fns, warmup, repeats))
        rec['ilqr_ms_per_step'] = rec['ilqr_backward']['median_ms'] / H
        if not args.only_ilqr:
            rec['ilqr_over_vjp'] = rec['ilqr_backward']['median_ms'] / rec['rollout_vjp']['median_ms']
            rec['baseline_over_ilqr'] = rec['linearize_then_torch']['median_ms'] / rec['ilqr_backward']['median_ms']
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        del b, act, traj, G
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/microbench/ilqr_cost.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)


if __name__ == '__main__':
    main()
