"""GPU checks of the batched extended Kalman filter (np_f16_model_ekf, F16Batch.ekf) against tests/test_ekf_cpu.py's fp64 restatement of
np_f16_ekf_io's definition, on test_gpu_linearize's flight conditions, and bit for bit against the rollout, against itself chained, and
against itself on other grids."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_ekf_cpu import SCALE, SENSORS, _inputs, _metric, _reference  # noqa: E402
from test_gpu_linearize import TOL_FACTOR, _batch, _same  # noqa: E402
from test_gpu_rollout_vjp import _dev  # noqa: E402

# `_metric` (means, covariance, nis) of `_ekf_ref(torch.float32)` against its fp64 self on the 130 rows over three steps, worst kept row, per
# sensor set (test_ekf_cpu._floor(), no GPU needed).  Without the equilibration the same recipe gives 7.14e-5 and 9.59e-5 for the covariance.
FLOOR = {SENSORS: (1.7308e-4, 2.9922e-6, 1.2492e-4), 0: (1.3228e-4, 8.3185e-7, 0.0), 0xFFFF: (1.0077e-4, 3.0160e-6, 6.1186e-5)}
TOL = {k: [TOL_FACTOR * x for x in v] for k, v in FLOOR.items()}
_CACHE = {}


def _run(n, H, measure, rows=None, edit=None, b=None, **kw):
    """the device on the first n rows (or `rows`) over H steps -> cpu tensors, row-major; edit(s, u, P0, act, z, r) changes the inputs in place"""
    s, u, P0, act, z, q, r = (np.array(x) for x in _inputs(n, H))
    if edit:
        edit(s, u, P0, act, z, r)
    if rows is not None:
        s, u, P0, act, z = s[rows], u[rows], P0[rows], act[:, rows], z[:, rows]
    out = (b or _batch()).ekf(_dev(act), _dev(z.transpose(0, 2, 1)) if measure else None, _dev(P0.transpose(1, 2, 0)), q, r, measure, s=_dev(s.T), u=_dev(u.T),
                              scale=SCALE, want_traj=True, **kw)
    s1, u1, P1, status, xt, pd, nis = (x.cpu() for x in out)
    return dict(x=torch.cat((s1, u1[:4])).t(), lef=u1[4], P=P1.permute(2, 0, 1), status=status, xt=xt.transpose(1, 2), pd=pd.transpose(1, 2), nis=nis)


def _clean(n, H, measure=SENSORS):
    if (n, H, measure) not in _CACHE:
        _CACHE[n, H, measure] = _run(n, H, measure)
    return _CACHE[n, H, measure]


def _take(o, rows):
    return {k: v[:, rows] if k in ('xt', 'pd', 'nis') else v[rows] for k, v in o.items()}


def _equal(a, b):
    return all(_same(a[k], b[k]) for k in a)


def _within(o, n, H, measure):
    xr, Pr, nisr, keep = _reference(measure)
    m = _metric(o['x'], o['P'], o['nis'][H - 1], xr[H - 1, :n], Pr[H - 1, :n], nisr[H - 1, :n])[:, keep[:n]].amax(1).tolist()
    print(f'n = {n}, H = {H}, measure {measure:#06x}: worst (mean, P, nis) on {int(keep[:n].sum())} rows ' + ', '.join(f'{x:.3e}' for x in m) + ' (tol ' + ', '.join(f'{x:.3e}' for x in TOL[measure]) + ')')
    return all(x <= t for x, t in zip(m, TOL[measure]))


@pytest.mark.parametrize('n,H', [(n, H) for n in (1, 9, 65, 130) for H in (1, 3)])
def test_against_the_fp64_filter(n, H):
    o = _clean(n, H)
    assert _reference(SENSORS)[3][0], 'row 0 is kept: n = 1 compares something'
    assert (o['status'] == -1).all() and _same(o['xt'][H - 1], o['x']) and _same(o['pd'][H - 1], torch.diagonal(o['P'], dim1=1, dim2=2))
    assert _same(o['lef'], _inputs(n, H)[1][:, 4]) and _within(o, n, H, SENSORS)


def test_without_a_sensor_the_mean_is_the_rollouts_bit_for_bit():
    n, H = 65, 3
    s, u, _, act = _inputs(n, H)[:4]
    s_end, u_end = _batch().rollout(_dev(act), _dev(s.T), _dev(u.T))
    o = _clean(n, H, 0)
    assert _same(o['x'], torch.cat((s_end, u_end[:4])).t().cpu()) and (o['nis'] == 0).all() and _within(o, n, H, 0)


def test_with_every_coordinate_measured():
    assert _within(_clean(65, 3, 0xFFFF), 65, 3, 0xFFFF)


def test_a_nan_sample_is_the_launch_without_that_sensor():
    def drop(s, u, P0, act, z, r):
        z[0, :, 4] = np.nan
    assert _equal(_run(65, 1, SENSORS, edit=drop), _run(65, 1, SENSORS & ~(1 << 4)))


def test_three_steps_are_three_chained_launches():
    n, b, whole = 65, _batch(), _clean(65, 3)
    s, u, P0, act, z, q, r = _inputs(n, 3)
    est = (_dev(s.T), _dev(u.T), _dev(P0.transpose(1, 2, 0)))
    for t in range(3):
        *est, status, xt, pd, nis = b.ekf(_dev(act[t:t + 1]), _dev(z[t:t + 1].transpose(0, 2, 1)), est[2], q, r, SENSORS, s=est[0], u=est[1], scale=SCALE, want_traj=True)
        assert (status == -1).all() and _same(xt[0].t().cpu(), whole['xt'][t]) and _same(pd[0].t().cpu(), whole['pd'][t]) and _same(nis[0].cpu(), whole['nis'][t])
    assert _same(torch.cat((est[0], est[1][:4])).t().cpu(), whole['x']) and _same(est[2].permute(2, 0, 1).cpu(), whole['P'])


@pytest.mark.parametrize('max_groups', [0, 1, 2])
def test_a_row_does_not_depend_on_where_it_lands(max_groups):
    full, alone = _run(130, 3, SENSORS, max_groups=max_groups), _run(130, 3, SENSORS, rows=slice(37, 38))
    assert _equal(full, _clean(130, 3)) and _equal(_take(full, slice(37, 38)), alone)


@pytest.mark.parametrize('case', ['nan_alpha', 'nan_in_p0', 'tiny_r'])
def test_edge_rows(case):
    n, H, e = 65, 3, 21

    def edit(s, u, P0, act, z, r):
        if case == 'nan_alpha':
            s[e, 7] = np.nan
        elif case == 'nan_in_p0':
            P0[e, 3, 5] = P0[e, 5, 3] = np.nan
        else:
            r[4] = 1e-12 * SCALE[4] ** 2
    o = _run(n, H if case != 'tiny_r' else 1, SENSORS, edit=edit)
    if case == 'tiny_r':   # r is the launch's: every row's estimate lands on its sample
        z = torch.from_numpy(_inputs(n, 1)[4][0, :, 4])
        miss = ((o['x'][:, 4].double() - z).abs() / SCALE[4]).max().item()
        print(f'worst distance to the sample: {miss:.3e} (tol {TOL[SENSORS][0]:.3e})')
        assert (o['status'] == -1).all() and miss <= TOL[SENSORS][0]
    else:   # one edited row: NaN, status -1; the others are those of the unedited launch, to the bit
        rest = [i for i in range(n) if i != e]
        assert _equal(_take(o, rest), _take(_clean(n, H), rest)) and o['status'][e] == -1 and torch.isnan(o['x'][e]).all() and torch.isnan(o['P'][e]).all()
        assert torch.isnan(o['xt'][:, e]).all() and torch.isnan(o['nis'][:, e]).all() and o['lef'][e] == _inputs(n, H)[1][e, 4]


@pytest.mark.parametrize('what,match', [('fleet', 'fleet'), ('gemm', 'aero_gemm_order'), ('tables', 'aero_1d_tables'), ('rk4', 'rk4'), ('combat', 'SingleCombat')])
def test_contexts_without_a_filter_are_refused_by_name(what, match):
    from neuralplane_amd.core import F16Batch, F16CombatBatch
    from neuralplane_amd.envs.utils.utils import parse_config
    kw = {'fleet': dict(airframes=[{}, {'mass': 700}]), 'gemm': dict(aero_gemm_order=True), 'tables': dict(aero_1d_tables=True), 'rk4': dict(solver='rk4')}.get(what, {})
    b = F16CombatBatch(4, parse_config('selfplay'), 'cuda:0') if what == 'combat' else _batch(8, **kw)
    z = lambda *shape: torch.zeros(shape, device='cuda')  # noqa: E731
    with pytest.raises(RuntimeError, match=match):
        F16Batch.ekf(b, z(2, 8, 4), z(2, 16, 8), z(16, 16, 8), np.ones(16), np.ones(16), SENSORS, s=z(12, 8), u=z(5, 8))
