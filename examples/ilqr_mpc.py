#!/usr/bin/env python3
"""iLQR on the F-16 model, every heavy step one launch: rollout -> cost gradients in torch -> ilqr_backward -> ilqr_forward with the whole
line search (alphas = 1, 1/2, ..., 2^-7) -> gather by `best`; rows whose sweep stopped or whose line search found nothing raise their mu.

    python examples/ilqr_mpc.py [--n 4096] [--horizon 50] [--iters 8]

The task: hold the start's altitude + 200 ft and its speed with the wings level, from the reset state, under a diagonal quadratic cost.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--horizon', type=int, default=50)
    ap.add_argument('--iters', type=int, default=8)
    args = ap.parse_args()
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    n, H, dev = args.n, args.horizon, 'cuda'
    b = F16Batch(n, parse_config('heading'), 'heading', 'cuda:0', seed=1)
    b.reset(want_obs=False)
    s0, u0 = b.s.clone(), b.u.clone()
    # the cost: 1/2 sum h_s (s - s_ref)^2 + 1/2 sum h_a a^2 on altitude, roll, pitch, speed and the body rates, in their own units
    w = torch.zeros(12)
    w[2], w[3], w[4], w[6], w[9:] = 1 / 100.0 ** 2, 1 / 0.1 ** 2, 1 / 0.1 ** 2, 1 / 10.0 ** 2, 1 / 0.2 ** 2
    h_s, h_a = w.repeat(H, 1), torch.full((4,), 1e-2)
    target = s0.clone()
    target[2] += 200.0
    target[3] = 0.0
    s_ref = target.repeat(H, 1, 1)
    hs_d, ha_d = h_s.to(dev), h_a.to(dev)
    alphas = [2.0 ** -i for i in range(8)]
    L, rows = len(alphas), torch.arange(n, device=dev)
    act, mu = torch.zeros((H, n, 4), device=dev), torch.full((n,), 1e-3, device=dev)
    for it in range(args.iters):
        traj = b.rollout(act, s0, u0, record_every=1)[2]
        e, a = traj - s_ref, act.clamp(-1, 1)
        cost_now = 0.5 * (hs_d[:, :, None] * e ** 2).sum((0, 1)) + 0.5 * (ha_d * a ** 2).sum((0, 2))
        k, K, dV, status = b.ilqr_backward(act, traj, hs_d[:, :, None] * e, (ha_d * a).transpose(1, 2), h_s, h_a, mu, s=s0, u=u0)
        act_new, _, _, _, cost, best = b.ilqr_forward(act, traj, k, K, alphas, s=s0, u=u0, cost=(h_s, h_a, s_ref))
        pick = rows * L + best.clamp(min=0)
        ok = (status < 0) & (best >= 0) & (cost[pick] < cost_now)
        act = torch.where(ok[None, :, None], act_new[:, pick], act)
        mu = torch.where(ok, (mu * 0.5).clamp(min=1e-6), mu * 10.0)
        print(f'iteration {it}: mean cost {torch.where(ok, cost[pick], cost_now).mean().item():.4f} (was {cost_now.mean().item():.4f}), '
              f'{int(ok.sum())} of {n} rows stepped, mean alpha {torch.tensor(alphas, device=dev)[best.clamp(min=0)][ok].mean().item():.3f}')


if __name__ == '__main__':
    main()
