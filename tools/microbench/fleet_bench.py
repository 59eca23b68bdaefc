"""Cost of per-row airframes: kernel time per env.step of a fleet context (K = 1 and K = 3 mixed inside every wave) against a one-airframe
context pinned to the throughput variant — the kernel shape the fleet kernels share — in one session, interleaved over rounds.

    python tools/microbench/fleet_bench.py [--rounds 3] [--steps 200] [--solver euler] [n ...]       (default n: 1000000 10000)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, '.')
from neuralplane_amd.envs.control_env import ControlEnv  # noqa: E402

CLASSES = [{}, {'mass': 700, 'Jy': 60000}, {'xcg': 0.25, 'S': 320.0, 'thrust_max': 60000.0, 'atm_lapse': 0.65e-5}]


def measure(n, kw, steps, solver):
    env = ControlEnv(num_envs=n, config='heading', model='F16', random_seed=0, device='cuda:0', solver=solver, **kw)
    env._batch.set_kernel_variant('throughput')
    env.reset()
    a = torch.rand(n, 4, device='cuda') * 0.4 - 0.2
    for _ in range(20):
        env.step(a)
    env._batch.set_timing(True)
    for _ in range(steps):
        env.step(a)
    torch.cuda.synchronize()
    s = env._batch.get_timing_samples()
    return statistics.median(s) * 1e3, min(s) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('sizes', nargs='*', type=int)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--solver', default='euler')
    args = ap.parse_args()
    cases = [('one airframe, throughput variant', {}), ('fleet K=1', {'airframes': CLASSES[:1]}), ('fleet K=3 mixed', {'airframes': CLASSES})]
    for n in args.sizes or [1_000_000, 10_000]:
        res = {name: [] for name, _ in cases}
        for _ in range(args.rounds):
            for name, kw in cases:
                res[name].append(measure(n, kw, args.steps, args.solver))
        base = min(m for m, _ in res[cases[0][0]])
        for name, _ in cases:
            med = [m for m, _ in res[name]]
            print(f'N={n} {args.solver} {name:34s} median us per round {" ".join(f"{m:.1f}" for m in med)}  best {min(med):.1f}  x{min(med) / base:.3f} of the one-airframe kernel', flush=True)


if __name__ == '__main__':
    main()
