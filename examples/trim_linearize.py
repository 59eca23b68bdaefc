#!/usr/bin/env python3
"""Trim a batch of F-16s for straight-and-level flight with Newton steps on the analytic linearisation, then read the short-period mode
off the trimmed A matrix.  Unknowns (alpha, theta, T, el); residuals xdot[6, 7, 10] (vt, alpha, Q rates) and the flight-path condition
theta - alpha = 0 (level flight at beta = phi = 0).

    python examples/trim_linearize.py [n]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralplane_amd.core import F16Batch  # noqa: E402
from neuralplane_amd.envs.utils.utils import parse_config  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=0)
s = torch.zeros((12, n), device='cuda')
u = torch.zeros((5, n), device='cuda')
s[2] = torch.linspace(5000.0, 25000.0, n)      # altitude, ft
s[6] = torch.linspace(400.0, 800.0, n)         # airspeed, ft/s
s[7] = s[4] = 0.05
u[0] = 3000.0
rows = [6, 7, 10]
for it in range(12):
    xdot, A, B = b.linearize(s, u)             # planar: xdot [12, n], A [12, 12, n], B [12, 4, n]
    r = torch.stack([xdot[6], xdot[7], xdot[10], s[4] - s[7]], 1)                                   # [n, 4]
    J = torch.zeros((n, 4, 4), device='cuda')
    J[:, :3, 0], J[:, :3, 1] = A[rows, 7].t(), A[rows, 4].t()                                        # d/d alpha, d/d theta
    J[:, :3, 2], J[:, :3, 3] = B[rows, 0].t(), B[rows, 1].t()                                        # d/d T, d/d el
    J[:, 3, 0], J[:, 3, 1] = -1.0, 1.0
    step = torch.linalg.solve(J, -r)
    s[7] += step[:, 0]
    s[4] += step[:, 1]
    u[0] += step[:, 2]
    u[1] += step[:, 3]
    print(f'newton step {it}: worst residual {r.abs().max().item():.3e}')
xdot, A, _ = b.linearize(s, u)
sp = A[[7, 10]][:, [7, 10]].permute(2, 0, 1)   # the (alpha, Q) block: the short-period approximation
eig = torch.linalg.eigvals(sp.cpu())
for k in range(n):
    print(f'alt {s[2, k].item():7.0f} ft  vt {s[6, k].item():5.0f} ft/s  alpha {s[7, k].item() * 57.2958:6.2f} deg  T {u[0, k].item():7.0f} lbf  '
          f'el {u[1, k].item():6.2f} deg  short period {eig[k, 0].real.item():+.3f} {eig[k, 0].imag.item():+.3f}j')
