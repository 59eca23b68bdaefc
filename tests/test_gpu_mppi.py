"""GPU checks of the MPPI step (np_f16_model_mppi, F16Batch.mppi): the candidates against the oracle's normals (to the bit), the fused cost
against the open-loop rollout of those candidates, and the re-weighting against fp64 softmin weights, teacher-forced on the device's own
costs and candidates."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ilqr import _cost  # noqa: E402
from test_gpu_linearize import W, _batch  # noqa: E402
from test_gpu_rollout_vjp import _dev, _inputs  # noqa: E402

H, SIGMA, SEED, CALL0 = 4, 0.3, 11, 5
# (P, K): aligned; several problems per wave with a ragged tail; no power of two, problems that straddle waves and the 128-row tile edge;
# a problem that spans workgroups and gives a lane of the update kernel more than one candidate
CASES = [(5, 64), (37, 8), (9, 48), (3, 200)]
GRID = [(P, K, shape, hold) for P, K in CASES for shape in ('throughput', 'split') for hold in (1, 2)]
_PROB, _RUN = {}, {}


def _problem(P):
    """P problems: a start, a plan within +-0.8 and a cost whose reference lies near the plan's own flight; once per size"""
    if P not in _PROB:
        s, u, act = _inputs(P, H)[:3]
        hs, ha = _cost(P, H)[1:]
        b, sd, ud, ad = _batch(), _dev(s.T), _dev(u.T), _dev(act * np.float32(0.8 / 1.2))
        traj = b.rollout(ad, sd, ud, record_every=1)[2]
        s_ref = traj + _dev((1e-2 * W.numpy()[:12, None] * np.random.RandomState(5).standard_normal((H, 12, P))).astype(np.float32))
        _PROB[P] = dict(b=b, s=sd, u=ud, act=ad, cost=(hs, ha, s_ref))
    return _PROB[P]


def _run(P, K, shape, hold, dead=None):
    """(T, plan, cost, best, ess, candidates) at the temperature the launch's own costs set: the median over the problems of (mean - min), so
    that the weights are neither uniform nor one-hot.  dead: s_ref of that problem is NaN, at the clean launch's temperature"""
    key = (P, K, shape, hold, dead)
    if key not in _RUN:
        p = _problem(P)
        hs, ha, s_ref = p['cost']
        if dead is not None:
            s_ref = s_ref.clone()
            s_ref[:, :, dead] = float('nan')
        kw = dict(cost=(hs, ha, s_ref), candidates=K, s=p['s'], u=p['u'], seed=SEED, call0=CALL0, hold=hold, shape=shape, want_candidates=True)
        if dead is None:
            c = p['b'].mppi(p['act'], SIGMA, 1.0, **kw)[1].view(P, K)   # the costs do not depend on the temperature
            T = np.float32((c.mean(1) - c.min(1).values).median().item())
        else:
            T = _run(P, K, shape, hold)[0]
        _RUN[key] = (T,) + p['b'].mppi(p['act'], SIGMA, float(T), **kw)
    return _RUN[key]


@pytest.mark.parametrize('hold', [1, 2])
@pytest.mark.parametrize('P,K', CASES)
def test_the_candidates_are_the_oracles_normals_about_the_plan_in_both_shapes(P, K, hold):
    """actions_out = clamp(fma(sigma, eps, abar)) to the bit.  The fma is formed in fp64, where the product is exact; the sum would have to land
    exactly on a float32 tie for the second rounding to matter"""
    from oracle.f16_oracle import rng_normals_rows
    a, b = _run(P, K, 'throughput', hold), _run(P, K, 'split', hold)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), 'the two shapes differ'
    eps = np.stack([rng_normals_rows(SEED, CALL0 + t // hold, 0, P * K)[:, :4] for t in range(H)]).astype(np.float64)
    eps[:, ::K] = 0.0   # candidate 0 flies the plan
    abar = _problem(P)['act'].cpu().numpy()
    raw = (float(np.float32(SIGMA)) * eps + np.repeat(abar, K, 1).astype(np.float64)).astype(np.float32)
    flown = a[5].cpu().numpy()
    assert np.array_equal(flown, np.clip(raw, -1, 1)) and np.array_equal(flown[:, ::K], np.clip(abar, -1, 1))
    assert (np.abs(raw) > 1).any() and not (np.abs(raw) > 1).all()


@pytest.mark.parametrize('P,K,shape,hold', GRID)
def test_the_cost_is_that_of_the_open_loop_rollout_of_the_candidates(P, K, shape, hold):
    p, out = _problem(P), _run(P, K, shape, hold)
    hs, ha, s_ref = p['cost']
    traj = p['b'].rollout(out[5], p['s'], p['u'], fanout=K, record_every=1)[2]
    e = traj.double().cpu() - s_ref.double().cpu().repeat_interleave(K, 2)
    ref = 0.5 * (torch.from_numpy(hs).double()[:, :, None] * e ** 2).sum((0, 1)) + 0.5 * (torch.from_numpy(ha).double() * out[5].double().cpu() ** 2).sum((0, 2))
    rel = ((out[2].double().cpu() - ref).abs() / ref).max().item()
    print(f'P={P} K={K} {shape} hold={hold}: worst relative cost error = {rel:.3e}')
    assert rel <= (16 * H + 4) * 2.0 ** -23


@pytest.mark.parametrize('P,K,shape,hold', GRID)
def test_the_update_against_fp64_softmin_teacher_forced(P, K, shape, hold):
    """First-order rounding, u = 2^-24, x_c = (cost_c - cmin) / T, L = ceil(log2 K) + 1 roundings along any path of a sum of K terms:
      a weight: x_c carries two roundings (the difference, the quotient), 2 u x_c on exp(-x_c), and the fp64 exp rounded once is within 2 u:
            rw_c = (2 x_c + 2) u;   the sum S: sum_c w_c rw_c / S + L u;   a normalised weight (one division): rel_c = rw_c + rS + u
      plan = sum_c w_c a_c: sum_c w_c rel_c |a_c|, the products' rounding and the sum's, (L + 1) u sum_c w_c |a_c|, and 2^-126 per weight
            that underflows;   ess = 1 / sum_c w_c^2: the squares' 2 rel_c weighted by w_c^2, a square, the sum and the reciprocal, (L + 2) u"""
    T, plan, cost, best, ess, flown = _run(P, K, shape, hold)
    c, a = cost.double().cpu().view(P, K), flown.double().cpu().view(H, P, K, 4)
    x = (c - c.min(1, keepdim=True).values) / float(T)
    w = torch.exp(-x) / torch.exp(-x).sum(1, keepdim=True)
    u, L = 2.0 ** -24, math.ceil(math.log2(K)) + 1
    rw = (2 * x + 2) * u
    rel = rw + ((w * rw).sum(1, keepdim=True) + L * u) + u
    mean = lambda wt, v: torch.einsum('pk,hpkj->hpj', wt, v)  # noqa: E731
    err_plan = (plan.double().cpu() - mean(w, a)).abs() / (mean(w * rel, a.abs()) + (L + 1) * u * mean(w, a.abs()) + K * 2.0 ** -126)
    ess_ref = 1 / (w ** 2).sum(1)
    err_ess = (ess.double().cpu() - ess_ref).abs() / (ess_ref * ((2 * rel * w ** 2).sum(1) * ess_ref + (L + 2) * u))
    worst = max(err_plan.max().item(), err_ess.max().item())
    print(f'P={P} K={K} {shape} hold={hold}: T = {T:.4g}, ess {ess.min().item():.2f} .. {ess.max().item():.2f}, worst error / bound = {worst:.3f}')
    assert worst <= 1.0 and torch.equal(best.cpu().long(), c.argmin(1)) and (plan.abs() <= 1).all()


@pytest.mark.parametrize('P,K,shape,hold', GRID)
def test_a_dead_problem_keeps_its_plan_and_touches_nobody(P, K, shape, hold):
    """s_ref is NaN for problem 3 (problem 0 where there are only three)"""
    q = 3 % P
    clean, dead = _run(P, K, shape, hold), _run(P, K, shape, hold, dead=q)
    T, plan, cost, best, ess, flown = dead
    assert torch.isnan(cost.view(P, K)[q]).all() and best[q] == -1 and ess[q] == 0
    assert torch.equal(plan[:, q], _problem(P)['act'][:, q, :4].clamp(-1, 1))
    others = torch.arange(P, device=plan.device) != q
    assert torch.equal(plan[:, others], clean[1][:, others]) and torch.equal(cost.view(P, K)[others], clean[2].view(P, K)[others])
    assert torch.equal(best[others], clean[3][others]) and torch.equal(ess[others], clean[4][others]) and torch.equal(flown, clean[5])


def test_one_candidate_is_the_plan_and_the_batch_is_left_as_it_was():
    p = _problem(37)
    b = p['b']
    b.reset(want_obs=False)
    was = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}, b.call_idx, b._version
    plan, cost, best, ess = b.mppi(p['act'], SIGMA, 0.5, cost=p['cost'], candidates=1, s=p['s'], u=p['u'])
    assert torch.equal(plan, p['act'][..., :4].clamp(-1, 1)) and (best == 0).all() and (ess == 1).all() and b.mppi_call == H
    now = b.state_dict()
    assert all(torch.equal(v, now[k]) if torch.is_tensor(v) else v == now[k] for k, v in was[0].items()) and (b.call_idx, b._version) == was[1:]


def test_an_rk4_context_is_refused_by_name_before_anything_is_launched():
    p = _problem(5)
    with pytest.raises(RuntimeError, match='rk4'):
        _batch(8, solver='rk4').mppi(p['act'], SIGMA, 0.5, cost=p['cost'], candidates=8, s=p['s'], u=p['u'])
