#!/usr/bin/env python3
"""LQG on the flight model: trim level flight over a grid of speeds and altitudes (F16Batch.trim), solve the steady-state LQR at every
operating point (F16Batch.lqr), then fly the regulators from NOISY measurements: every step the extended Kalman filter (F16Batch.ekf) turns
the sample into an estimate, and the feedback law (F16Batch.ilqr_forward, one step, k = 0 and the constant K) acts on the estimate, not on
the truth.  The normalised innovation squared is printed against its expectation, the number of sensors.

    python examples/ekf_lqg.py [n] [H]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralplane_amd.core import LQR_NO_POSITION_HEADING, F16Batch, trim_problem  # noqa: E402
from neuralplane_amd.envs.utils.utils import parse_config  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
H = int(sys.argv[2]) if len(sys.argv) > 2 else 500
b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=0)
s = torch.zeros((12, n), device='cuda')
u = torch.zeros((5, n), device='cuda')
s[2] = torch.linspace(5000.0, 25000.0, n)      # altitude, ft
s[6] = torch.linspace(400.0, 800.0, n)         # airspeed, ft/s
s[7] = s[4] = 0.05
u[0] = 3000.0
unknowns, rows, scale, lo, hi = trim_problem('longitudinal')
st, ut, _, _, trim_status, _, A, B = b.trim(s, u, unknowns, rows, scale=scale, lo=lo, hi=hi, want_linearization=True)
h_s = [0.0, 0.0, 1e-4, 100.0, 100.0, 0.0, 1e-2, 1e3, 1e3, 10.0, 10.0, 10.0]
K, _, _, lqr_status = b.lqr(A, B, h_s, [1.0] * 4, select=LQR_NO_POSITION_HEADING)
print(f'trim: {int((trim_status == 0).sum())} of {n} converged; lqr: {int((lqr_status == 0).sum())} of {n} converged')

# the sensors: altitude, attitude, airspeed and body rates, with their 1-sigma errors; alpha, beta and the lagged controls are not measured
sensors = [2, 3, 4, 5, 6, 9, 10, 11]
measure = sum(1 << k for k in sensors)
sigma = torch.ones(16, device='cuda')
sigma[2], sigma[3:6], sigma[6], sigma[9:12] = 20.0, 0.01, 2.0, 0.005
r = (sigma ** 2).tolist()
q = [1e-2, 1e-2, 1e-2, 1e-8, 1e-8, 1e-8, 1e-4, 1e-8, 1e-8, 1e-7, 1e-7, 1e-7, 1e-2, 1e-6, 1e-6, 1e-6]   # what the model does not know, per step
P = torch.diag(torch.tensor([1e2, 1e2, 1e4, 1e-3, 1e-3, 1e-3, 1e2, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e2, 1e-2, 1e-2, 1e-2], device='cuda'))[:, :, None].repeat(1, 1, n)

gain = torch.tensor([0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5], device='cuda')
a_hold = (0.1 * ut[:4] / gain[:, None]).t().contiguous()[None]   # the action that holds the trimmed controls against the lag, [1, n, 4]
zero_k, K1, s_ref = torch.zeros((1, 4, n), device='cuda'), K[None], st[None]
truth_s, truth_u = st.clone(), ut.clone()
truth_s[2] += 100.0                                                # the truth starts 100 ft high, 10 ft/s slow and 3 deg banked;
truth_s[6] -= 10.0                                                 # the filter starts at the operating point and does not know
truth_s[3] += 0.05
est_s, est_u = st.clone(), ut.clone()
gen = torch.Generator(device='cuda').manual_seed(1)
nis_sum = torch.zeros(n, device='cuda')
for t in range(H):
    act = b.ilqr_forward(a_hold, s_ref, zero_k, K1, [1.0], s=st, u=ut, s_init=est_s, u_init=est_u)[0]   # [1, n, 4]: the law on the estimate
    truth_s, truth_u = b.rollout(act, truth_s, truth_u)
    z = torch.full((1, 16, n), float('nan'), device='cuda')
    z[0, sensors] = torch.cat((truth_s, truth_u[:4]))[sensors] + sigma[sensors, None] * torch.randn((len(sensors), n), device='cuda', generator=gen)
    est_s, est_u, P, status, _, _, nis = b.ekf(act, z, P, q, r, measure, s=est_s, u=est_u, want_traj=True)
    nis_sum += nis[0]
print(f'filter: {int((status == -1).sum())} of {n} rows ran through; mean NIS {nis_sum.mean().item() / H:.2f} (expected {len(sensors)})')
for k in range(n):
    print(f'  alt {st[2, k].item():7.0f} ft  vt {st[6, k].item():5.0f} ft/s  after {H * 0.02:.0f} s: truth off trim by {truth_s[2, k].item() - st[2, k].item():+7.2f} ft '
          f'{truth_s[6, k].item() - st[6, k].item():+6.2f} ft/s  phi {truth_s[3, k].item():+.4f} rad;  estimate off truth by '
          f'{est_s[2, k].item() - truth_s[2, k].item():+6.2f} ft {est_s[6, k].item() - truth_s[6, k].item():+5.2f} ft/s  alpha {est_s[7, k].item() - truth_s[7, k].item():+.5f} rad')
