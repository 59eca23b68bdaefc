#!/usr/bin/env python3
"""Receding-horizon MPPI on the fused call: one `env.model.mppi(...)` per control step.

    python examples/mppi_mpc.py [--n 256] [--k 64] [--horizon 20] [--iters 5]

The loop of examples/lookahead_mppi.py — every aircraft carries a plan [H, 4], K perturbed copies are flown from its CURRENT state, the
plan moves towards the cheap ones, the first action is flown — with everything between "plan in" and "plan out" inside the library:
the noise is drawn in registers from the env's counter-based generator, the cost ("hold altitude and speed, wings level", as a diagonal
about a reference) is accumulated while flying, and the softmin average makes the candidates again instead of reading them.  No noise,
candidate or trajectory tensor exists, and the env's own random stream is not advanced.
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
    h_s = torch.zeros((H, 12))                                       # cost = 1/2 sum h_s (s - s_ref)^2 + 1/2 sum h_a a^2, per step
    h_s[:, 2], h_s[:, 6], h_s[:, 3] = 2 / 100.0 ** 2, 2 / 20.0 ** 2, 2.0   # altitude [ft], speed [ft/s], bank [rad]
    h_a = torch.full((4,), 1e-2)
    for it in range(args.iters):
        s_ref = env.model.s.clone()                                  # [n, 12]: hold the current altitude and speed ...
        s_ref[:, 3] = 0.0                                            # ... wings level
        plan, cost, best, ess = env.model.mppi(plan, 0.2, 0.5 * H, cost=(h_s, h_a, s_ref.expand(H, n, 12)), candidates=K)
        env.step(plan[0])                                            # fly the first action; the env's own state advances only here
        plan = torch.cat([plan[1:], plan[-1:]], 0)                   # receding horizon
        c = cost.view(n, K)
        print(f'step {it}: mean candidate cost {c.mean().item():.4f}, best {c.min(1).values.mean().item():.4f}, '
              f'effective samples {ess.mean().item():.1f} of {K}, problems without a finite candidate {(best < 0).sum().item()}')


if __name__ == '__main__':
    main()
