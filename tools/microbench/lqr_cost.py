#!/usr/bin/env python3
"""What a batched LQR costs (F16Batch.lqr, np_f16_model_lqr) at n = 3 000, 65 536 and 10^6 level-flight trim points, against the routes it
replaces: the same doubling in torch on the GPU (bmm + torch.linalg.solve, run for as many doublings as the call's slowest row took) and, at
n = 3 000, scipy.linalg.solve_discrete_are per row on the host.  HIP-event medians in one process; writes profiles/lqr_cost.json.

    python tools/microbench/lqr_cost.py [--reps 7] [--out profiles/lqr_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from neuralplane_amd.core import LQR_NO_POSITION_HEADING, F16Batch, trim_problem  # noqa: E402
from neuralplane_amd.envs.utils.utils import parse_config  # noqa: E402

DT, KAPPA, GAIN = 0.02, 0.9, (0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5)
H_S = [1.0, 1.0, 1e-6, 100.0, 100.0, 100.0, 1e-2, 1e4, 1e4, 100.0, 100.0, 100.0]   # one over the square of a typical excursion
H_A = [1.0, 1.0, 1.0, 1.0]


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def step_map(A, B, select):
    """(A_d, B_d, Q, R) [n, 16, 16], [n, 16, 4], [16, 16], [4, 4] from the planar A, B (include/neuralplane_amd.h: np_f16_lqr_io), unequilibrated"""
    n, dev = A.shape[2], A.device
    m = torch.tensor([(select >> k) & 1 for k in range(16)], dtype=torch.float32, device=dev)
    Phi = torch.eye(16, device=dev).repeat(n, 1, 1)
    Phi[:, :12] += DT * torch.cat((A, B), 1).permute(2, 0, 1)
    S = torch.tensor([1.0] * 12 + [KAPPA] * 4, device=dev)
    return (m[:, None] * (Phi * S) * m, m[:, None] * Phi[:, :, 12:] * torch.tensor(GAIN, device=dev),
            torch.diag(torch.tensor(H_S + [0.0] * 4, device=dev) * m), torch.diag(torch.tensor(H_A, device=dev)))


def torch_route(A, B, select, doublings):
    Ad, Bd, Q, R = step_map(A, B, select)
    eye = torch.eye(16, device=A.device)
    Ak, G, H = Ad, Bd @ torch.linalg.solve(R, Bd.transpose(1, 2)), Q.repeat(A.shape[2], 1, 1)
    for _ in range(doublings):
        XY = torch.linalg.solve(eye + G @ H, torch.cat((Ak, G), 2))
        X, Y = XY[:, :, :16], XY[:, :, 16:]
        M, N = Ak.transpose(1, 2) @ H @ X, Ak @ Y @ Ak.transpose(1, 2)
        Ak, G, H = Ak @ X, G + 0.5 * (N + N.transpose(1, 2)), H + 0.5 * (M + M.transpose(1, 2))
    BtH = Bd.transpose(1, 2) @ H
    return -torch.linalg.solve(R + BtH @ Bd, BtH @ Ad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='+', default=[3000, 65536, 1000000])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lqr_cost.json'))
    args = ap.parse_args()
    b = F16Batch(8, parse_config('heading'), 'heading', 'cuda:0', seed=0)
    unknowns, rows, scale, lo, hi = trim_problem('longitudinal')
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'select': LQR_NO_POSITION_HEADING, 'h_s': H_S, 'h_a': H_A, 'sizes': {}}
    for n in args.sizes:
        s, u = torch.zeros((12, n), device='cuda'), torch.zeros((5, n), device='cuda')
        k = torch.arange(n, device='cuda')
        s[2], s[6], s[7], s[4], u[0] = 5000.0 + 20000.0 * (k % 1000) / 1000.0, 400.0 + 400.0 * (k // 1000) / max(n // 1000, 1), 0.05, 0.05, 3000.0
        *_, A, B = b.trim(s, u, unknowns, rows, scale=scale, lo=lo, hi=hi, want_linearization=True)
        K, doublings, _, status = b.lqr(A, B, H_S, H_A, select=LQR_NO_POSITION_HEADING)
        d = int(doublings.max())
        rec = {'converged': int((status == 0).sum()), 'doublings_min': int(doublings.min()), 'doublings_max': d, 'doublings_mean': doublings.float().mean().item()}
        rec['lqr_ms'] = median_ms(lambda: b.lqr(A, B, H_S, H_A, select=LQR_NO_POSITION_HEADING), args.reps)
        rec['lqr_with_P_ms'] = median_ms(lambda: b.lqr(A, B, H_S, H_A, select=LQR_NO_POSITION_HEADING, want_P=True), args.reps)
        rec['torch_doubling_ms'] = median_ms(lambda: torch_route(A, B, LQR_NO_POSITION_HEADING, d), max(args.reps // 2, 3))
        Kt = torch_route(A, B, LQR_NO_POSITION_HEADING, d).permute(1, 2, 0)
        rec['torch_vs_call_max_rel'] = ((Kt - K).abs().amax((0, 1)) / K.abs().amax((0, 1))).max().item()
        if n <= 3000:
            from scipy.linalg import solve_discrete_are
            sel = [i for i in range(16) if (LQR_NO_POSITION_HEADING >> i) & 1]
            Ad, Bd, Q, R = (x.double().cpu().numpy() for x in step_map(A, B, LQR_NO_POSITION_HEADING))
            t0 = time.perf_counter()
            for i in range(n):
                solve_discrete_are(Ad[i][sel][:, sel], Bd[i][sel], Q[sel][:, sel], R)
            rec['scipy_host_ms'] = (time.perf_counter() - t0) * 1e3
        out['sizes'][str(n)] = rec
        print(n, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
