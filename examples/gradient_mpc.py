#!/usr/bin/env python3
"""Gradient shooting with the differentiable rollout: Adam on an action sequence, the gradient from one fused reverse sweep.

    python examples/gradient_mpc.py [--n 256] [--horizon 20] [--iters 30]

The gradient counterpart of lookahead_mppi.py: instead of K sampled candidates per aircraft, `env.model.rollout_diff(plan)` returns the
trajectory of ONE plan per aircraft and `loss.backward()` runs `np_f16_model_rollout_vjp` — one launch — for d cost / d plan.  The start is
perturbed (a bank and a heading offset), the cost is "hold altitude and heading, wings level".  The env itself is never stepped.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--iters', type=int, default=30)
    args = ap.parse_args()
    from neuralplane_amd.envs.control_env import ControlEnv
    env = ControlEnv(num_envs=args.n, config='heading', model='F16', random_seed=0, device='cuda:0')
    env.reset()
    s0, u0 = env.model.s.clone(), env.model.u.clone()               # [n, 12], [n, 5]
    alt0, psi0 = s0[:, 2].clone(), s0[:, 5].clone()
    s0[:, 3] += 0.2                                                  # start banked ...
    s0[:, 5] += 0.05                                                 # ... and off heading
    plan = torch.zeros((args.horizon, args.n, 4), device=s0.device)
    plan[:, :, 0] = 0.3
    plan.requires_grad_(True)
    opt = torch.optim.Adam([plan], lr=0.05)
    for it in range(args.iters):
        opt.zero_grad()
        traj, _ = env.model.rollout_diff(plan, s0, u0)              # [H, n, 12]
        cost = (((traj[:, :, 2] - alt0) / 10.0) ** 2 + ((traj[:, :, 5] - psi0) / 0.05) ** 2 + (traj[:, :, 3] / 0.2) ** 2).mean()
        cost.backward()                                              # one reverse-sweep launch
        opt.step()
        print(f'iteration {it}: cost {cost.item():.5f}')


if __name__ == '__main__':
    main()
