"""GPU checks of the batched LQR (np_f16_model_lqr, F16Batch.lqr) against tests/test_lqr_cpu.py's fp64 restatement of the doubling, on the
fp32-rounded Jacobians of test_gpu_linearize's flight conditions: both sides see the same A and B, so only the solver is measured."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_linearize import TOL_FACTOR, _batch  # noqa: E402
from test_lqr_cpu import LONGITUDINAL, NO_POS_HEADING, _lqr_ref, _metric, _problem, _rows  # noqa: E402

# `_metric` of `_lqr_ref(torch.float32)` against its fp64 self on these 130 rows with positions and heading deselected, worst row
# (test_lqr_cpu._floor(), no GPU needed): 4.0734e-4 with the equilibration; without it the same recipe gives 4.52e-2.
TOL_FP32_SELF = 4.0734e-4
TOL = TOL_FACTOR * TOL_FP32_SELF
# the same recipe with all 16 coordinates selected on the edge test's 65 rows (the integrators make it worse conditioned): 1.0113e-3
TOL_ALL = TOL_FACTOR * 1.0113e-3
WAVES = 4   # per workgroup (csrc/np_model_lqr.h)
_CACHE = {}


def _lqr(J, hs, ha, b=None, **kw):
    """J [n, 12, 16] -> (K [n, 4, 16], P [n, 16, 16], doublings, res, status) on the cpu"""
    Jd = J.cuda().permute(1, 2, 0).contiguous()
    K, doublings, res, status, P = (b or _batch()).lqr(Jd[:, :12].contiguous(), Jd[:, 12:].contiguous(), hs, ha, want_P=True, **kw)
    return K.permute(2, 0, 1).cpu(), P.permute(2, 0, 1).cpu(), doublings.cpu(), res.cpu(), status.cpu()


def _clean(n, select):
    if (n, select) not in _CACHE:
        J, hs, ha = _rows(n)
        _CACHE[n, select] = (_lqr(J, hs, ha, select=select), _lqr_ref(torch.float64, J, hs, ha, select))
    return _CACHE[n, select]


@pytest.mark.parametrize('n', [1, WAVES + 1, 130])
def test_against_the_fp64_doubling(n):
    (K, P, doublings, res, status), (Kr, Pr, dr, _, sr) = _clean(n, NO_POS_HEADING)
    m = _metric(K, P, Kr, Pr)
    print(f'n = {n}: worst metric {m.max().item():.3e} (tol {TOL:.3e}), doublings {int(doublings.min())}..{int(doublings.max())}, worst res {res.max().item():.2e}')
    assert (sr == 0).all() and (status == 0).all() and ((doublings - dr).abs() <= 1).all() and m.max().item() <= TOL


@pytest.mark.parametrize('max_groups', [0, 1, 2])
def test_a_row_does_not_depend_on_where_it_lands(max_groups):
    J, hs, ha = _rows(130)
    alone, full = _lqr(J[37:38], hs, ha, select=NO_POS_HEADING), _lqr(J, hs, ha, select=NO_POS_HEADING, max_groups=max_groups)
    assert all(torch.equal(x[0], y[37]) for x, y in zip(alone, full)) and all(torch.equal(x, y) for x, y in zip(full, _clean(130, NO_POS_HEADING)[0]))


@pytest.mark.parametrize('case', ['nan_in_a', 'b_zero', 'longitudinal', 'no_doublings', 'all_selected'])
def test_edge_rows(case):
    J, hs, ha = _rows(65)
    J, e, kw = J.clone(), 21, dict(select=LONGITUDINAL if case == 'longitudinal' else 0xFFFF if case == 'all_selected' else NO_POS_HEADING)
    if case == 'nan_in_a':
        J[e, 7, 10] = float('nan')
    elif case == 'b_zero':
        Ad = _problem(J, hs, ha, NO_POS_HEADING, torch.float64)[0]
        e = int(torch.linalg.eigvals(Ad[:, :12, :12]).abs().amax(1).argmax())   # the row whose weighted states have the most unstable mode
        assert torch.linalg.eigvals(Ad[e, :12, :12]).abs().max() > 1
        J[e, :, 12:] = 0
    elif case == 'no_doublings':
        kw['max_doublings'] = 0
    K, P, doublings, res, status = out = _lqr(J, hs, ha, **kw)
    if case in ('nan_in_a', 'b_zero'):   # one edited row: the others are those of the unedited launch, to the bit
        rest = [i for i in range(65) if i != e]
        assert all(torch.equal(x[rest], y[rest]) for x, y in zip(out, _clean(65, NO_POS_HEADING)[0]))
    if case == 'nan_in_a':
        assert status[e] == 4 and torch.isnan(K[e]).all() and torch.isnan(P[e]).all()
    elif case == 'b_zero':
        print(f'status {int(status[e])} after {int(doublings[e])} doublings, res {res[e].item():.2e}')
        assert status[e] != 0 and torch.isfinite(K[e]).all() and torch.isfinite(P[e]).all()
    elif case == 'longitudinal':
        off = [k for k in range(16) if not (LONGITUDINAL >> k) & 1]
        Kr, Pr = _lqr_ref(torch.float64, J, hs, ha, LONGITUDINAL)[:2]
        assert (status == 0).all() and (K[:, :, off] == 0).all() and (P[:, off] == 0).all() and (P[:, :, off] == 0).all() and _metric(K, P, Kr, Pr).max().item() <= TOL
    elif case == 'no_doublings':   # the one-step gain of H_0 = Q, against the formula: three chained products of at most 16 terms, 8 x 20 x 2^-24 = 1e-5
        Ad, Bd, Q, R = _problem(J, hs, ha, NO_POS_HEADING, torch.float64)
        Kr = -torch.linalg.solve(R + Bd.transpose(1, 2) @ Q @ Bd, Bd.transpose(1, 2) @ Q @ Ad)
        assert (status == 1).all() and (doublings == 0).all() and _metric(K, P, Kr, Q.repeat(65, 1, 1)).max().item() <= 1e-5
    else:   # with the position and heading integrators in: the limit, or convergence with the reference agreeing
        Kr, Pr, _, _, sr = _lqr_ref(torch.float64, J, hs, ha, 0xFFFF)
        conv = status == 0
        print(f'{int(conv.sum())} of 65 converged; worst metric on them {_metric(K, P, Kr, Pr)[conv].max().item():.3e}')
        assert ((status == 0) | (status == 1)).all() and (sr[conv] == 0).all() and _metric(K, P, Kr, Pr)[conv].max().item() <= TOL_ALL


def test_trim_to_lqr_stabilises_every_operating_point():
    from neuralplane_amd.core import LQR_NO_POSITION_HEADING, trim_problem
    from test_gpu_ilqr import _cost
    n, b = 65, _batch()
    s, u = torch.zeros((12, n), device='cuda'), torch.zeros((5, n), device='cuda')
    s[2], s[6], s[7], s[4], u[0] = torch.linspace(5000.0, 25000.0, n), torch.linspace(400.0, 800.0, n), 0.05, 0.05, 3000.0
    unknowns, rows, scale, lo, hi = trim_problem('longitudinal')
    *_, trim_status, _, A, B = b.trim(s, u, unknowns, rows, scale=scale, lo=lo, hi=hi, want_linearization=True)
    _, hs, ha = _cost(1, 1)
    K, _, _, status = b.lqr(A, B, hs[0], ha, select=LQR_NO_POSITION_HEADING)
    Ad, Bd = _problem(torch.cat((A, B), 1).permute(2, 0, 1).cpu(), hs[0], ha, NO_POS_HEADING, torch.float64)[:2]
    rho = torch.linalg.eigvals(Ad + Bd @ K.permute(2, 0, 1).cpu().double()).abs().amax(1)
    print(f'spectral radius of the closed loop: {rho.min().item():.6f}..{rho.max().item():.6f}')
    assert (trim_status == 0).all() and (status == 0).all() and (rho < 1).all()


@pytest.mark.parametrize('what,match', [('fleet', 'fleet'), ('rk4', 'rk4'), ('combat', 'SingleCombat')])
def test_contexts_without_this_step_map_are_refused_by_name(what, match):
    from neuralplane_amd.core import F16Batch, F16CombatBatch
    from neuralplane_amd.envs.utils.utils import parse_config
    kw = {'fleet': dict(airframes=[{}, {'mass': 700}]), 'rk4': dict(solver='rk4')}.get(what, {})
    b = F16CombatBatch(4, parse_config('selfplay'), 'cuda:0') if what == 'combat' else _batch(8, **kw)
    with pytest.raises(RuntimeError, match=match):
        F16Batch.lqr(b, torch.zeros((12, 12, 8), device='cuda'), torch.zeros((12, 4, 8), device='cuda'), np.ones(12, np.float32), np.ones(4, np.float32))
