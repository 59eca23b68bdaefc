#!/usr/bin/env python3
"""A gain schedule in three launches: trim level flight over a grid of speeds and altitudes (F16Batch.trim), solve the steady-state LQR at
every operating point (F16Batch.lqr, positions and heading deselected), and fly the regulators from perturbed starts (F16Batch.ilqr_forward
with k = 0 and the constant K expanded over the horizon).

    python examples/lqr_schedule.py [n] [H]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralplane_amd import _lib  # noqa: E402
from neuralplane_amd.core import LQR_NO_POSITION_HEADING, F16Batch, trim_problem  # noqa: E402
from neuralplane_amd.envs.utils.utils import parse_config  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
H = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=0)
s = torch.zeros((12, n), device='cuda')
u = torch.zeros((5, n), device='cuda')
s[2] = torch.linspace(5000.0, 25000.0, n)      # altitude, ft
s[6] = torch.linspace(400.0, 800.0, n)         # airspeed, ft/s
s[7] = s[4] = 0.05
u[0] = 3000.0
unknowns, rows, scale, lo, hi = trim_problem('longitudinal')
st, ut, _, _, trim_status, _, A, B = b.trim(s, u, unknowns, rows, scale=scale, lo=lo, hi=hi, want_linearization=True)

# the cost: one over the square of a tolerable excursion per state (ft, rad, ft/s, rad/s), unit weight on the normalised actions
h_s = [0.0, 0.0, 1e-4, 100.0, 100.0, 0.0, 1e-2, 1e3, 1e3, 10.0, 10.0, 10.0]
K, doublings, res, status = b.lqr(A, B, h_s, [1.0] * 4, select=LQR_NO_POSITION_HEADING)
print(f'trim: {int((trim_status == 0).sum())} of {n} converged; lqr: {int((status == 0).sum())} of {n} converged in {int(doublings.min())}..{int(doublings.max())} doublings')

# the reference is the operating point itself, held at every step, with the action that holds the trimmed controls against the lag
# (u' = 0.9 u + 0.1 scale a); positions and heading have zero gain columns, so their reference does not matter
gain = torch.tensor([0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5], device='cuda')
a_hold = (0.1 * ut[:4] / gain[:, None]).t().contiguous()                 # [n, 4]
actions = a_hold.repeat(H, 1, 1)
s_traj = st.repeat(H, 1, 1)
s0 = st.clone()
s0[2] += 100.0                                                           # 100 ft high,
s0[6] -= 10.0                                                            # 10 ft/s slow,
s0[7] += 0.02                                                            # and 1.1 deg of alpha and 3 deg of bank off trim
s0[3] += 0.05
flown = b.ilqr_forward(actions, s_traj, torch.zeros((H, 4, n), device='cuda'), K.repeat(H, 1, 1, 1), [1.0], s=st, u=ut, s_init=s0, u_init=ut.clone())
s_end = flown[1]
for k in range(n):
    print(f'  alt {st[2, k].item():7.0f} ft  vt {st[6, k].item():5.0f} ft/s  {_lib.LQR_STATUS[int(status[k])]:>10}  after {H * 0.02:.0f} s: '
          f'd alt {s_end[2, k].item() - st[2, k].item():+7.2f} ft  d vt {s_end[6, k].item() - st[6, k].item():+6.2f} ft/s  '
          f'd alpha {s_end[7, k].item() - st[7, k].item():+.4f} rad  phi {s_end[3, k].item():+.4f} rad')
