#!/usr/bin/env python3
"""Look-ahead with the open-loop model rollout: one MPPI-style update of an action plan per control step.

    python examples/lookahead_mppi.py [--n 256] [--k 64] [--horizon 20] [--iters 5]

Every aircraft carries a nominal action sequence [H, 4].  Per control step K perturbed copies of it are rolled out from the aircraft's
CURRENT state — `env.model.rollout(a_seq, fanout=K)`: one launch, no K copies of the state, the env untouched — a cost is read off the
recorded trajectory, and the plan moves towards the cheap candidates (softmin weights).  The point is the call, not the controller: the
cost is "hold altitude and speed, wings level".
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--k', type=int, default=64)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--iters', type=int, default=5)
    args = ap.parse_args()
    from neuralplane_amd.envs.control_env import ControlEnv
    n, K, H = args.n, args.k, args.horizon
    env = ControlEnv(num_envs=n, config='heading', model='F16', random_seed=0, device='cuda:0')
    env.reset()
    dev = env.model.s.device
    plan = torch.zeros((H, n, 4), device=dev)
    plan[:, :, 0] = 0.3                                              # some throttle to start from
    gen = torch.Generator(device=dev).manual_seed(0)
    for it in range(args.iters):
        s_now = env.model.s                                          # [n, 12]; (npos, epos, alt, phi, theta, psi, vt, ...)
        alt0, vt0 = s_now[:, 2].repeat_interleave(K), s_now[:, 6].repeat_interleave(K)
        noise = 0.2 * torch.randn((H, n * K, 4), device=dev, generator=gen)
        cand = (plan.repeat_interleave(K, dim=1) + noise).clamp(-1, 1)   # row r = candidate r % K of aircraft r // K
        _, _, traj = env.model.rollout(cand, fanout=K, record_every=5)   # traj [H // 5, n * K, 12]
        cost = (((traj[:, :, 2] - alt0) / 100.0) ** 2 + ((traj[:, :, 6] - vt0) / 20.0) ** 2 + traj[:, :, 3] ** 2).mean(0)
        cost = torch.nan_to_num(cost, nan=1e6, posinf=1e6)
        w = torch.softmax(-(cost.view(n, K) - cost.view(n, K).min(1, keepdim=True).values) / 0.5, dim=1)      # [n, K]
        plan = (w.t().reshape(1, K, n, 1) * cand.view(H, n, K, 4).transpose(1, 2)).sum(1)
        env.step(plan[0])                                            # fly the first action; the env's own state advances only here
        plan = torch.cat([plan[1:], plan[-1:]], 0)                   # receding horizon
        print(f'step {it}: mean candidate cost {cost.mean().item():.4f}, best {cost.view(n, K).min(1).values.mean().item():.4f}')


if __name__ == '__main__':
    main()
