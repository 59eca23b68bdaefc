"""GPU parity of the open-loop model rollout (np_f16_model_rollout, F16Batch.rollout): H applications of F16Model.update in one launch,
bit for bit (==, or both NaN) against the CPU oracle's Oracle.update called H times and against H update launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.f16_oracle import Oracle  # noqa: E402  (the checker; test infrastructure)

SOLVERS = [None, 'rk4']
# one lane; one 64-row tile plus a row; two 128-row tiles plus a ragged 37 rows, with a record stride that does not divide the horizon
CASES = [(1, 1, 0), (65, 2, 1), (293, 7, 3)]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _batch(n, solver=None, task='heading', airframe=None, **kw):
    from neuralplane_amd.core import F16Batch
    from neuralplane_amd.envs.utils.utils import parse_config
    cfg = parse_config(task)
    if airframe:
        cfg.airframe = airframe
    return F16Batch(n, cfg, task, 'cuda:0', seed=3, solver=solver, **kw)


_REFS = {}


def _reference(solver, n, H, airframe=None):
    """(rand_u of the reset, actions [H, n, 4], oracle states after every step [H, n, 12], controls at the end [n, 5]); once per case"""
    key = (solver, n, H, bool(airframe))
    if key not in _REFS:
        rng = np.random.RandomState(17 + n + H)
        o = Oracle('heading', solver=solver, overrides={'airframe': dict(airframe)} if airframe else None)
        st = Oracle.new_state(n)
        ru = rng.uniform(0, 1, (n, 5)).astype(np.float32)
        o.reset(st, rand_u=ru, want_obs=False)
        a = rng.uniform(-1.5, 1.5, (H, n, 4)).astype(np.float32)   # beyond +-1: the clamp acts
        if n > 8:
            a[:, n // 2] = np.nan
            a[:, n - 3] = [np.inf, -np.inf, np.inf, -np.inf]
        states = []
        for t in range(H):
            o.update(st, a[t])
            states.append(st['s'].copy())
        _REFS[key] = (ru, a, np.stack(states), st['u'].copy())
    return _REFS[key]


def _start(n, solver, ru, **kw):
    b = _batch(n, solver, **kw)
    b.reset(rand_u=torch.from_numpy(ru), want_obs=False)
    return b


@pytest.mark.parametrize('n,H,every', CASES)
@pytest.mark.parametrize('solver,shape', [(s, sh) for s in SOLVERS for sh in ('auto', 'throughput', 'split') if not (s == 'rk4' and sh == 'split')])
def test_rollout_equals_the_oracle_and_the_update_launches(solver, shape, n, H, every):
    ru, a, states, u_end = _reference(solver, n, H)
    b = _start(n, solver, ru)
    out = b.rollout(torch.from_numpy(a).cuda(), record_every=every, shape=shape)
    s, u = out[0].cpu().numpy().T, out[1].cpu().numpy().T
    assert _same(s, states[-1]) and _same(u, u_end), 'rollout differs from Oracle.update applied H times'
    twin = _start(n, solver, ru)
    for t in range(H):
        twin.update(torch.from_numpy(a[t]).cuda())
    assert _same(s, twin.s.cpu().numpy().T) and _same(u, twin.u.cpu().numpy().T), 'rollout differs from H update launches'
    if every:
        traj = out[2].cpu().numpy()
        assert traj.shape == (H // every, 12, n)
        for j in range(H // every):
            assert _same(traj[j].T, states[(j + 1) * every - 1]), f'record {j} differs from the oracle state after step {(j + 1) * every}'
    if n > 8:
        assert np.isnan(s[n // 2]).all() and np.isfinite(s[[n // 2 - 1, n // 2 + 1, n - 4, n - 2]]).all()


def test_held_action_equals_the_repeated_sequence():
    n, H = 293, 5
    ru, a, _, _ = _reference(None, n, 7)
    b = _start(n, None, ru)
    held = b.rollout(torch.from_numpy(a[0]).cuda(), horizon=H, record_every=2)
    seq = b.rollout(torch.from_numpy(np.repeat(a[:1], H, 0)).cuda(), record_every=2)
    assert all(_same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(held, seq)) and held[2].shape == (2, 12, n)


def test_fanout_row_r_starts_from_row_r_over_k():
    n0, K, H = 37, 3, 4
    ru = np.random.RandomState(1).uniform(0, 1, (n0, 5)).astype(np.float32)
    a = torch.from_numpy(np.random.RandomState(2).uniform(-1.5, 1.5, (H, n0 * K, 4)).astype(np.float32)).cuda()
    b = _start(n0, None, ru)
    fan = b.rollout(a, fanout=K, record_every=2)
    src = torch.arange(n0 * K, device='cuda') // K
    one = b.rollout(a, s=b.s[:, src], u=b.u[:, src], record_every=2)   # the same starts, copied out in torch
    assert fan[0].shape == (12, n0 * K) and all(_same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(fan, one))
    assert not _same(fan[0][:, 0].cpu().numpy(), fan[0][:, 1].cpu().numpy()), 'rows of one aircraft follow their own actions'


@pytest.mark.parametrize('shape', ['throughput', 'split'])
def test_rollout_leaves_the_batch_as_it_was(shape):
    n = 293
    ru, a, _, _ = _reference(None, n, 7)
    b, twin = _start(n, None, ru), _start(n, None, ru)
    act = torch.from_numpy(a[0]).cuda().nan_to_num(0.0, 1.0, -1.0)
    for x in (b, twin):
        x.step(act)                      # the cross-step coefficient cache is live from here on
    keep = [t.clone() for t in (b.s, b.u, b.flags, b.step_count, b.tgt)] + [b.call_idx]
    b.rollout(torch.from_numpy(a).cuda(), record_every=3, shape=shape)
    now = [b.s, b.u, b.flags, b.step_count, b.tgt, b.call_idx]
    assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(keep, now))
    got, want = b.step(act), twin.step(act)   # a disturbed coefficient cache would show here
    assert all(_same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want)) and _same(b.s.cpu().numpy(), twin.s.cpu().numpy())


@pytest.mark.parametrize('what,match', [('fleet', 'fleet'), ('gemm', 'aero_gemm_order'), ('tables', 'aero_1d_tables'), ('combat', 'SingleCombat'),
                                        ('rk4_split', 'Euler only'), ('horizon', 'horizon'), ('fanout', 'fanout')])
def test_refusals_name_the_cause(what, match):
    from neuralplane_amd.core import F16Batch, F16CombatBatch
    from neuralplane_amd.envs.utils.utils import parse_config
    n = 8
    kw = {'fleet': dict(airframes=[{}, {'mass': 700}]), 'gemm': dict(aero_gemm_order=True), 'tables': dict(aero_1d_tables=True), 'rk4_split': dict(solver='rk4')}.get(what, {})
    b = F16CombatBatch(n // 2, parse_config('selfplay'), 'cuda:0') if what == 'combat' else _batch(n, **kw)
    a = torch.zeros((n, 4), device='cuda')
    call = dict(horizon=0 if what == 'horizon' else 2, fanout=0 if what == 'fanout' else 1, shape='split' if what == 'rk4_split' else 'auto')
    with pytest.raises(RuntimeError, match=match):
        F16Batch.rollout(b, a, s=torch.zeros((12, n), device='cuda'), u=torch.zeros((5, n), device='cuda'), **call)


def test_airframe_as_data():
    n, H, af = 65, 3, {'mass': 700, 'Jy': 60000}
    ru, a, states, u_end = _reference(None, n, H, airframe=af)
    b = _start(n, None, ru, airframe=af)
    s, u = b.rollout(torch.from_numpy(a).cuda())
    assert _same(s.cpu().numpy().T, states[-1]) and _same(u.cpu().numpy().T, u_end)
    assert not _same(states[-1], _reference(None, n, H)[2][-1]), 'the airframe must matter, or this compares nothing'
