"""Bit-exactness of the pair (two and three waves per SIMD) and throughput Euler step kernels on small ragged batches: free-running steps
with auto-resets on tail lanes and partial tiles, state edits no version counter sees, env.reset / model.reset mid-run and a checkpoint
round trip.  Bar: HIP == oracle bit for bit at every step.  (Among much else these steps cover the observation's EAS2TAS, columns 8 and 21,
which takes the atmosphere power the Overload evaluation computed for the same altitude.)

A row's trajectory is a function of (seed, call index, global row) and its own actions only, so ONE oracle run per task at the largest batch
(257 rows) is the reference of every smaller batch (its first n rows).

The pair variant's build for three waves per SIMD — the N = 1e6 headline kernel — is chosen by grid size; at small sizes only the
process-wide NPF16_PAIR_WAVES=3 (include/neuralplane_amd.h), read once when the library first dispatches, selects it.  Its leg of the
matrix therefore runs in ONE child process started with that variable (this file run as a script).
"""
import os
import subprocess
import sys
import tempfile
import functools

import numpy as np
import pytest
import torch

if __name__ == '__main__':   # the child process of the three-waves leg: no conftest puts the repository root on the path
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.f16_oracle import Oracle  # noqa: E402  (the checker; test infrastructure)

SIZES = [1, 63, 64, 65, 129, 257]   # one lane, a wave minus / plus one lane, a tile plus one lane, two tiles plus one lane
N_MAX, STEPS, SEED = 257, 40, 1234
FIELDS = ('s', 'u', 'tgt', 'step_count', 'done', 'bad', 'timeout')


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _actions():
    """hazard-rich random actions (beyond the clamp, the elevator three times as far every seventh step): episodes end all along the run"""
    rng = np.random.RandomState(5)
    out = []
    for t in range(STEPS):
        a = rng.uniform(-1.5, 1.5, (N_MAX, 4)).astype(np.float32)
        a[:, 1] *= 3.0 if t % 7 == 0 else 1.0
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def _reference(task):
    """reset + STEPS free-running steps of the oracle at N_MAX rows, production RNG: per step (state dict, obs, reward), and the number of
    auto-resets (rows flagged by a step that a later step of the run re-initialises)"""
    o, st = Oracle(task), Oracle.new_state(N_MAX)
    o_obs = o.reset(st, seed=SEED, call_idx=0)
    traj = [({k: st[k].copy() for k in FIELDS}, o_obs.copy(), None)]
    resets = 0
    for t, a in enumerate(_actions()):
        o_obs, o_rew, _, _, _ = o.step(st, a, seed=SEED, call_idx=t + 1)
        traj.append(({k: st[k].copy() for k in FIELDS}, o_obs.copy(), o_rew.copy()))
        if t < STEPS - 1:
            resets += int((st['done'] | st['bad'] | st['timeout']).astype(bool).sum())
    return traj, resets


@pytest.mark.parametrize('task', ['heading', 'tracking'])
def test_reference_run_contains_auto_resets(task):
    """CPU: with this seed and these actions the oracle alone re-initialises 157 rows inside the 40 steps at 257 rows (either task: the
    overload and attitude limits end the episodes, not the task); without them the in-kernel reset path would not run."""
    _, resets = _reference(task)
    assert resets == 157, f'{task}: {resets} auto-resets in the reference run'


def test_cache_rows_and_abi_number():
    """CPU: np_f16_cache_floats reports 16 rows per aircraft (14 coefficients + the 2 keys), padded to whole 128-aircraft workgroups; the ABI number of the library is the binding's and the header's."""
    import os
    import re
    from neuralplane_amd import _lib, build
    build.build_hip()
    lib = _lib.load()
    rows = 14 + 2
    for n, padded in [(1, 128), (128, 128), (129, 256), (257, 384), (1_000_000, 1_000_064)]:
        assert lib.np_f16_cache_floats(n) == padded * rows, n
    assert lib.np_f16_cache_floats(0) == 0 and lib.np_f16_cache_floats(-5) == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'neuralplane_amd.h')).read()
    assert lib.np_abi_version() == _lib.ABI_VERSION == int(re.search(r'#define NP_ABI_VERSION (\d+)', header).group(1))


def _batch(task, n, variant):
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    b = F16Batch(n, parse_config(task), task, 'cuda:0', seed=SEED)
    b.set_kernel_variant(variant)
    return b


def _check(b, n, obs, rew, flags, ref, what):
    st, o_obs, o_rew = ref
    assert _same(b.s.cpu().numpy().T, st['s'][:n]), f'{what}: state differs from the oracle'
    assert _same(b.u.cpu().numpy().T, st['u'][:n]), f'{what}: controls differ'
    assert _same(b.tgt.cpu().numpy().T, st['tgt'][:n]), f'{what}: targets differ'
    assert np.array_equal(b.step_count.cpu().numpy(), st['step_count'][:n]), f'{what}: step_count differs'
    f = flags.cpu().numpy()
    assert np.array_equal(f[0], st['done'][:n]) and np.array_equal(f[1], st['bad'][:n]) and np.array_equal(f[2], st['timeout'][:n]), f'{what}: masks differ'
    assert _same(obs.cpu().numpy(), o_obs[:n]), f'{what}: obs differs'
    if rew is not None:
        assert _same(rew.cpu().numpy(), o_rew[:n]), f'{what}: reward differs'


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('variant', ['pair', 'throughput'])   # at these sizes the pinned pair variant is the two-waves-per-SIMD build
@pytest.mark.parametrize('task', ['heading', 'tracking'])
def test_free_running_with_auto_resets_bit_exact(task, variant, n):
    """reset + 40 steps of random actions on the production RNG, tail lanes, partial and several tiles: states, controls, targets, counters,
    observation, reward, flags equal the oracle's at every step."""
    _run_free(task, variant, n)


def _run_free(task, variant, n):
    traj, resets = _reference(task)
    assert resets >= 1
    b = _batch(task, n, variant)
    obs = b.reset()
    _check(b, n, obs, None, b.flags, traj[0], f'{task}/{variant}/{n}: reset')
    cached_steps = 0
    for t, a in enumerate(_actions()):
        cached_steps += int(b._cache_valid and b.s._version == b._s_version)
        obs, rew, flags = b.step(torch.from_numpy(a[:n].copy()).cuda())
        _check(b, n, obs, rew, flags, traj[t + 1], f'{task}/{variant}/{n}: step {t}')
    assert cached_steps == STEPS - 1, 'every step but the first must have run the cached kernel'


@pytest.mark.gpu
def test_three_waves_per_simd_pair_build_bit_exact():
    """The pair variant built for three waves per SIMD (the N = 1e6 headline kernel) is chosen by grid size only — more than four workgroups
    per CU: reset + 6 steps on such a batch with a ragged last tile (the oracle run is the cost: ~0.13 M rows x 6 steps)."""
    from neuralplane_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * cus * 128 + 257
    assert _lib.dispatch_plan(n, cus)['pair3'] == 1
    task, seed = 'heading', 77
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    b = F16Batch(n, parse_config(task), task, 'cuda:0', seed=seed)
    o, st = Oracle(task), Oracle.new_state(n)
    obs = b.reset()
    assert _same(obs.cpu().numpy(), o.reset(st, seed=seed, call_idx=0))
    rng = np.random.RandomState(3)
    for t in range(6):
        a = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
        if t == 3:   # invisible edits in the first, a middle and the ragged last tile: theta, altitude, phi
            for row, col, val in [(5, 4, 0.21), (70_001, 2, 4321.0), (n - 1, 3, -0.4)]:
                b.s.data[col, row] = val
                st['s'][row, col] = val
        obs, rew, flags = b.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _, _, _ = o.step(st, a, seed=seed, call_idx=t + 1)
        assert _same(b.s.cpu().numpy().T, st['s']), f'state differs at step {t}'
        assert _same(obs.cpu().numpy(), o_obs) and _same(rew.cpu().numpy(), o_rew), f'obs / reward differ at step {t}'
        f = flags.cpu().numpy()
        assert np.array_equal(f[0], st['done']) and np.array_equal(f[1], st['bad']) and np.array_equal(f[2], st['timeout'])


EDITS = {   # state column, new value
    'phi': (3, 0.35), 'theta': (4, -0.12), 'altitude': (2, 5555.5), 'alpha': (7, 0.09),
}


@pytest.mark.gpu
@pytest.mark.parametrize('what', sorted(EDITS))
@pytest.mark.parametrize('variant', ['pair', 'throughput'])
def test_invisible_state_edit_is_noticed(variant, what):
    """A write that bumps no version counter (`.data[...] =`) to phi, theta, the altitude or alpha, in rows of a full wave, of a partial
    tile and the batch's last row: the next step (still the cached kernel) equals the oracle stepping from the edited state bit for bit,
    and so do five more."""
    _run_edit(variant, what)


def _run_edit(variant, what):
    task, n, seed = 'heading', 257, SEED
    b = _batch(task, n, variant)
    o, st = Oracle(task), Oracle.new_state(n)
    rng = np.random.RandomState(21)
    obs = b.reset()
    assert _same(obs.cpu().numpy(), o.reset(st, seed=seed, call_idx=0))
    col, val = EDITS[what]
    rows = [0, 37, 64, 130, n - 1]
    for t in range(9):
        if t == 3:
            v0 = b.s._version
            for r in rows:
                b.s.data[col, r] = val
                st['s'][r, col] = val
            assert b.s._version == v0 and b._cache_valid, 'the edit must be invisible to the host-side check'
        a = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        obs, rew, flags = b.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _, _, _ = o.step(st, a, seed=seed, call_idx=t + 1)
        _check(b, n, obs, rew, flags, (st, o_obs, o_rew), f'{variant}/{what}: step {t}')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['pair', 'throughput'])
def test_reset_model_reset_and_checkpoint_mid_run(variant, tmp_path):
    """env.reset() and model.reset(env) in the middle of a run and a checkpoint save / load round trip into a fresh environment, each
    followed by five bit-exact steps."""
    _run_resets(variant, tmp_path)


def _run_resets(variant, tmp_path):
    from neuralplane_amd.envs.control_env import ControlEnv
    task, n, seed = 'tracking', 257, 31
    o, st = Oracle(task), Oracle.new_state(n)
    rng = np.random.RandomState(8)

    def make():
        e = ControlEnv(num_envs=n, config=task, model='F16', random_seed=seed, device='cuda:0')
        e._batch.set_kernel_variant(variant)
        return e

    env = make()
    call = 0

    def steps(e, k, what):
        nonlocal call
        for t in range(k):
            a = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
            obs, rew, done, bad, tmo, _ = e.step(torch.from_numpy(a).cuda())
            o_obs, o_rew, _, _, _ = o.step(st, a, seed=seed, call_idx=call)
            call += 1
            _check(e._batch, n, obs, rew, e._batch.flags, (st, o_obs, o_rew), f'{variant}: {what}, step {t}')

    assert _same(env.reset().cpu().numpy(), o.reset(st, seed=seed, call_idx=call))
    call += 1
    steps(env, 12, 'start')
    flagged = int((st['done'] | st['bad'] | st['timeout']).astype(bool).sum())
    assert _same(env.reset().cpu().numpy(), o.reset(st, seed=seed, call_idx=call))          # env.reset(): flagged rows re-initialised, flags cleared
    call += 1
    steps(env, 5, 'after env.reset')
    steps(env, 7, 'on')
    flagged += int((st['done'] | st['bad'] | st['timeout']).astype(bool).sum())
    env.model.reset(env)                                                                        # F16Model.reset alone: flags stay
    o.model_reset(st, seed=seed, call_idx=call)
    call += 1
    steps(env, 5, 'after model.reset')
    assert flagged > 0, 'no row was flagged at either reset: the reset kernel rewrote nothing'
    torch.save(env.state_dict(), os.path.join(tmp_path, 'env.pt'))
    env2 = make()
    env2.load_state_dict(torch.load(os.path.join(tmp_path, 'env.pt')))
    steps(env2, 5, 'after the checkpoint round trip')


@pytest.mark.gpu
def test_pair_three_waves_leg_in_child_process():
    """The same matrix for the pair variant's three-waves-per-SIMD build: sizes 1 .. 257 x {heading, tracking} free-running with auto-resets,
    the four invisible edits and the resets / checkpoint run, in one child process started with NPF16_PAIR_WAVES=3 (a fresh process: the
    library reads the variable once).  The child prints one line per case and a final count."""
    env = dict(os.environ, NPF16_PAIR_WAVES='3')
    r = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), '--pair3-child'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-4000:]
    assert f'pair3 child OK: {len(SIZES) * 2 + len(EDITS) + 1} cases' in r.stdout, r.stdout[-2000:]


def _pair3_child():
    assert os.environ.get('NPF16_PAIR_WAVES') == '3'
    cases = 0
    for task in ('heading', 'tracking'):
        for n in SIZES:
            _run_free(task, 'pair', n)
            cases += 1
            print(f'free-running {task} n={n} ok', flush=True)
    for what in sorted(EDITS):
        _run_edit('pair', what)
        cases += 1
        print(f'edit {what} ok', flush=True)
    with tempfile.TemporaryDirectory() as td:
        _run_resets('pair', td)
    cases += 1
    print(f'pair3 child OK: {cases} cases', flush=True)


if __name__ == '__main__' and '--pair3-child' in sys.argv:
    _pair3_child()
