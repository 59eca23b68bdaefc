"""GPU checks of iLQR's forward pass (np_f16_model_rollout_feedback, F16Batch.ilqr_forward): the feedback rollout under a real ilqr_backward's
gains against the open-loop rollout (to the bit) and against the law restated in fp64, teacher-forced on the device's own trajectory."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ilqr import MU, _cost  # noqa: E402
from test_gpu_linearize import W, _batch  # noqa: E402
from test_gpu_rollout_vjp import GAIN, LAG_KEEP, _dev, _inputs  # noqa: E402

H = 4
# (P, L): one ragged tile without sharing; 296 rows = three throughput tiles with a ragged tail, aligned groups; 135 rows, groups that
# straddle a wave and the 128-row tile edge (no `best`: L is no power of two)
CASES = [(37, 1), (37, 8), (45, 3)]
SHAPES = ['throughput', 'split']
_NOM, _FLY = {}, {}


def _nominal(P, h=H):
    """the nominal flight of P problems, a real ilqr_backward's gains about it, a perturbed start and a cost reference: once per size"""
    if (P, h) not in _NOM:
        s, u, act, G, gu = _inputs(P, h)
        ga, hs, ha = _cost(P, h)
        b, sd, ud, ad, r = _batch(), _dev(s.T), _dev(u.T), _dev(act), np.random.RandomState(5)
        traj = b.rollout(ad, sd, ud, record_every=1)[2]
        k, K = b.ilqr_backward(ad, traj, _dev(G.transpose(0, 2, 1)), _dev(ga.transpose(0, 2, 1)), hs, ha, MU, g_u_end=_dev(gu[:, :4].T), s=sd, u=ud)[:2]
        w = W.float().numpy()
        s_init = sd + _dev((1e-2 * w[:12, None] * r.standard_normal((12, P))).astype(np.float32))
        u_init = ud + _dev((1e-2 * np.r_[w[12:], 0][:, None] * r.standard_normal((5, P))).astype(np.float32))
        s_ref = traj + _dev((1e-2 * w[:12, None] * r.standard_normal((h, 12, P))).astype(np.float32))
        _NOM[P, h] = dict(b=b, s=sd, u=ud, act=ad, traj=traj, k=k.contiguous(), K=K.contiguous(), s_init=s_init, u_init=u_init, cost=(hs, ha, s_ref))
    return _NOM[P, h]


def _law(a0, alpha, k, K, x, xb):
    """the law in the dtype of its arguments, [4, n]: a = abar + alpha k + K (x - xbar), x = (s, u entering the step) [16, n]; and the sum of
    the magnitudes of its terms, which a first-order rounding bound multiplies"""
    return a0 + alpha * k + torch.einsum('ajr,jr->ar', K, x - xb), a0.abs() + (alpha * k).abs() + torch.einsum('ajr,jr->ar', K.abs(), x.abs() + xb.abs())


def _lag(u, a, gain=GAIN, keep=LAG_KEEP):
    """F16Model.update's control lag on an already clamped action, [4, n]"""
    return keep * u + gain[:, None] * a


def _fly(P, L, shape, h=H, nan=False):
    """the forward pass from the perturbed start with alphas = (1, 1/2, 1/4, ...) and the fused cost, once per case"""
    key = (P, L, shape, h, nan)
    if key not in _FLY:
        n, K = _nominal(P, h), _nominal(P, h)['K']
        if nan:
            K = K.clone()
            K[1, 0, 0, 3] = float('nan')
        _FLY[key] = n['b'].ilqr_forward(n['act'], n['traj'], n['k'], K, [2.0 ** -i for i in range(L)], s=n['s'], u=n['u'], s_init=n['s_init'],
                                        u_init=n['u_init'], cost=n['cost'], shape=shape, want_best=L & (L - 1) == 0)
    return _FLY[key]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('P,L', CASES)
def test_alpha_zero_from_the_nominal_start_is_the_nominal_flight(P, L, shape):
    n = _nominal(P)
    act, _, _, traj = n['b'].ilqr_forward(n['act'], n['traj'], n['k'], n['K'], [0.0] * L, s=n['s'], u=n['u'], shape=shape)
    assert (act == n['act'].clamp(-1, 1).repeat_interleave(L, 1)).all() and (traj == n['traj'].repeat_interleave(L, 2)).all()


@pytest.mark.parametrize('P,L,h', [c + (H,) for c in CASES] + [(37, 8, 1)])
def test_the_trajectory_is_the_open_loop_rollout_of_the_returned_actions_in_both_shapes(P, L, h):
    n, a, b = _nominal(P, h), _fly(P, L, 'throughput', h), _fly(P, L, 'split', h)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the two shapes differ'
    s_end, u_end, traj = n['b'].rollout(a[0], n['s_init'], n['u_init'], fanout=L, record_every=1)
    assert torch.equal(traj, a[3]) and torch.equal(s_end, a[1]) and torch.equal(u_end, a[2]) and torch.equal(a[3][-1], a[1])


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('P,L', CASES)
def test_the_law_against_fp64_teacher_forced(P, L, shape):
    n, out = _nominal(P), _fly(P, L, shape)
    d, rep = lambda x: x.double().cpu(), lambda x: x.double().cpu().repeat_interleave(L, -1)  # noqa: E731
    acts, abar, alpha = d(out[0]), d(n['act']).clamp(-1, 1), torch.tensor([2.0 ** -(r % L) for r in range(P * L)], dtype=torch.float64)
    x = torch.cat((rep(n['s_init']), rep(n['u_init'][:4])))   # [16, P L]
    xb = torch.cat((d(n['s']), d(n['u'][:4])))                 # [16, P]
    worst, clamps = 0.0, []
    for t in range(H):
        k, K, a0, xbr = rep(n['k'][t]), rep(n['K'][t]), rep(n['act'][t, :, :4].t()), xb.repeat_interleave(L, -1)
        raw, mag = _law(a0, alpha, k, K, x, xbr)
        worst = max(worst, ((acts[t].t() - raw.clamp(-1, 1)).abs() / (32 * 2.0 ** -24 * mag)).max().item())
        clamps.append(raw.abs() > 1)
        x = torch.cat((d(out[3][t]), _lag(x[12:], acts[t].t())))   # teacher-forced: the device's own state and actions
        xb = torch.cat((d(n['traj'][t]), _lag(xb[12:], abar[t, :, :4].t())))
    print(f'P={P} L={L} {shape}: worst error / bound = {worst:.3f}')
    clamps = torch.stack(clamps)
    assert worst <= 1.0 and clamps.any() and not clamps.all()


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('P,L', CASES)
def test_cost_and_best_and_a_nan_gain(P, L, shape):
    n, out, bad = _nominal(P), _fly(P, L, shape), _fly(P, L, shape, nan=True)
    hs, ha, s_ref = n['cost']
    e = out[3].double().cpu() - s_ref.double().cpu().repeat_interleave(L, 2)
    ref = 0.5 * (torch.from_numpy(hs).double()[:, :, None] * e ** 2).sum((0, 1)) + 0.5 * (torch.from_numpy(ha).double() * out[0].double().cpu() ** 2).sum((0, 2))
    rel = ((out[4].double().cpu() - ref).abs() / ref).max().item()
    print(f'P={P} L={L} {shape}: worst relative cost error = {rel:.3e}')
    assert rel <= (16 * H + 4) * 2.0 ** -23
    mine = slice(3 * L, 4 * L)   # problem 3 has a NaN in K_1: NaN cost, never chosen; every other row is that of the clean launch
    assert torch.isnan(bad[4][mine]).all() and torch.isnan(bad[3][-1, :, mine]).all()
    for x, y in zip(out[:5], bad[:5]):
        rows = x.dim() - 1 if x.dim() != 3 or x.shape[2] != 4 else 1
        keep = torch.ones(x.shape[rows], dtype=torch.bool)
        keep[mine] = False
        assert torch.equal(x.index_select(rows, keep.nonzero()[:, 0].cuda()), y.index_select(rows, keep.nonzero()[:, 0].cuda()))
    if L & (L - 1) == 0:
        for o in (out, bad):
            c = o[4].cpu().numpy().reshape(P, L)
            c = np.where(np.isfinite(c), c, np.inf)
            assert np.array_equal(o[5].cpu().numpy(), np.where(np.isinf(c).all(1), -1, c.argmin(1)))
        assert bad[5][3] == -1 and (out[5] >= 0).all()


def test_the_batch_is_left_as_it_was():
    n = _nominal(37)
    b = n['b']
    b.reset(want_obs=False)
    was = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}, b.call_idx, b._version
    b.ilqr_forward(n['act'], n['traj'], n['k'], n['K'], [1.0, 0.5], s=n['s'], u=n['u'], cost=n['cost'])
    now = b.state_dict()
    assert all(torch.equal(v, now[k]) if torch.is_tensor(v) else v == now[k] for k, v in was[0].items()) and (b.call_idx, b._version) == was[1:]


@pytest.mark.parametrize('what,match', [('rk4', 'rk4'), ('best', 'power of two'), ('alpha', r'alphas must be finite and in \[0, 1\]'), ('h_s', 'h_s must be finite and not negative')])
def test_refusals_by_name_before_anything_is_launched(what, match):
    n = _nominal(37)
    hs, ha, s_ref = n['cost']
    b = _batch(8, solver='rk4') if what == 'rk4' else n['b']
    alphas = {'best': [1.0, 0.5, 0.25], 'alpha': [1.0, 1.5]}.get(what, [1.0, 0.5])
    cost = (np.where(np.arange(12) == 7, -1e-6, hs).astype(np.float32), ha, s_ref) if what == 'h_s' else n['cost']
    with pytest.raises(RuntimeError, match=match):
        b.ilqr_forward(n['act'], n['traj'], n['k'], n['K'], alphas, s=n['s'], u=n['u'], cost=cost)
