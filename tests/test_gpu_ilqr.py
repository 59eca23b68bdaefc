"""GPU checks of iLQR's backward pass (np_f16_model_ilqr_backward, F16Batch.ilqr_backward): teacher-forced on the device's own trajectory against
the Riccati sweep restated in fp64 over the autograd Jacobians of the plain torch restatement of nlplant."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_linearize import F16, TOL_FACTOR, W, _batch, _jac  # noqa: E402
from test_gpu_rollout_vjp import DT, GAIN, LAG_KEEP, MAX_EXCLUDED, _dev, _inputs, _kept  # noqa: E402
from test_gpu_rollout_vjp import TOL as VJP_TOL, _metric as _vjp_metric  # noqa: E402

# `_metric` of `_sweep` run in torch.float32 on the CPU against its fp64 self, on the accuracy test's input (256 rows, H = 4, the oracle's
# trajectory), worst kept row: 5.8324e-6, with 0.152 of the rows excluded (`_floor()` returns both; tests/test_ilqr_cpu.py runs it, no GPU needed).
TOL_FP32_SELF = 5.8324e-6
TOL = TOL_FACTOR * TOL_FP32_SELF
MU = 1e-3


def _riccati(Phi, D, G, ga, gu, hs, ha, mu, kappa=LAG_KEEP):
    """The sweep of include/neuralplane_amd.h (np_f16_ilqr_io), term by term, in the dtype of Phi [H, n, 16, 16]: D [H, n, 4], G [H, n, 12],
    ga [H, n, 4], gu [n, 4], hs [H, 12], ha [4], mu [n] -> k [H, n, 4], K [H, n, 4, 16], dV [n, 2], status [n], p0 [n, 16], P0 [n, 16, 16]"""
    dt, (H, n) = Phi.dtype, Phi.shape[:2]
    z4, eye4 = torch.zeros((n, 4), dtype=dt), torch.eye(4, dtype=dt)
    p, P = torch.cat((torch.zeros((n, 12), dtype=dt), gu), 1), torch.zeros((n, 16, 16), dtype=dt)
    S = torch.cat((torch.ones(12, dtype=dt), kappa * torch.ones(4, dtype=dt)))
    k, K, dV, status = torch.zeros((H, n, 4), dtype=dt), torch.zeros((H, n, 4, 16), dtype=dt), torch.zeros((n, 2), dtype=dt), torch.full((n,), -1)
    for t in reversed(range(H)):
        p, P = p + torch.cat((G[t], z4), 1), P + torch.diag_embed(torch.cat((hs[t], z4[0])))
        F, Dm = Phi[t], D[t]
        w, Wm = torch.einsum('nij,ni->nj', F, p), F.transpose(1, 2) @ P @ F
        Qx, Qa = S * w, Dm * w[:, 12:] + ga[t]
        Qxx, Qax = S[:, None] * Wm * S, Dm[:, :, None] * Wm[:, 12:] * S
        Qaa = Dm[:, :, None] * Wm[:, 12:, 12:] * Dm[:, None] + torch.diag_embed(ha)
        Qt = Qaa + mu[:, None, None] * eye4
        bad = (torch.linalg.cholesky_ex(Qt).info != 0) | ~torch.isfinite(Qa).all(1) | ~torch.isfinite(Qt).all(2).all(1)
        status[bad & (status < 0)] = t
        live = status < 0
        Qs = torch.where(live[:, None, None], Qt, eye4)
        kt, Kt = -torch.linalg.solve(Qs, torch.where(live[:, None], Qa, z4)[:, :, None])[:, :, 0], -torch.linalg.solve(Qs, torch.where(live[:, None, None], Qax, torch.zeros_like(Qax)))
        Qk = torch.einsum('nab,nb->na', Qaa, kt)
        dV = dV + torch.where(live[:, None], torch.stack(((kt * Qa).sum(1), 0.5 * (kt * Qk).sum(1)), 1), torch.zeros_like(dV))
        KT = Kt.transpose(1, 2)
        pn = Qx + torch.einsum('nja,na->nj', KT, Qk) + torch.einsum('nja,na->nj', KT, Qa) + torch.einsum('naj,na->nj', Qax, kt)
        Pn = Qxx + KT @ Qaa @ Kt + KT @ Qax + Qax.transpose(1, 2) @ Kt
        k[t], K[t] = torch.where(live[:, None], kt, z4), torch.where(live[:, None, None], Kt, torch.zeros_like(Kt))
        p, P = torch.where(live[:, None], pn, p), torch.where(live[:, None, None], 0.5 * (Pn + Pn.transpose(1, 2)), P)
    live = status < 0
    return k, K, dV * live[:, None], status, p * live[:, None], P * live[:, None, None]


def _rows_of(out, idx):
    """the rows `idx` of (k [H, n, 4], K [H, n, 4, 16], dV, status, p0, P0)"""
    return tuple(x[:, idx] if j < 2 else x[idx] for j, x in enumerate(out))


def _cost(n, H, seed=23):
    """the cost model beside `_inputs`: direct action gradients, Gauss-Newton diagonals of order one in W's units, h_a = 1"""
    r = np.random.RandomState(seed)
    return r.standard_normal((H, n, 4)).astype(np.float32), (r.uniform(0.5, 1.5, (H, 12)) / W[:12].numpy() ** 2).astype(np.float32), np.ones(4, np.float32)


def _sweep(dtype, S, U, act, G, ga, gu, hs, ha, mu, af=F16):
    """S [H, n, 12] = s_0..s_{H-1}, U [H, n, 5] = u_1..u_H: Phi from the autograd Jacobians in `dtype`, then `_riccati`"""
    n, T = S[0].shape[0], lambda x: torch.from_numpy(np.asarray(x)).to(dtype)  # noqa: E731
    Phi = torch.eye(16, dtype=dtype).repeat(len(S), n, 1, 1)
    for t in range(len(S)):
        Phi[t, :, :12] += DT * _jac(dtype, S[t], U[t], af)[1]
    a = T(act)
    D = torch.where((a >= -1) & (a <= 1), GAIN.to(dtype), torch.zeros((), dtype=dtype))
    return _riccati(Phi, D, T(G), T(ga), T(gu)[:, :4], T(hs), T(ha), torch.as_tensor(mu, dtype=dtype).expand(n))


def _ratio(err, ref):
    """err / ref, an output whose reference is all zero (the gain row of a clamped action) counting as 0 if it is zero too and as inf if not"""
    return torch.where(ref == 0, torch.where(err == 0, 0.0, float('inf')).double(), err / ref)


def _metric(out, ref):
    """per row, the worst of: k over its H x 4 entries, K and P0 per output in W's units, p0 in W's units, dV relative"""
    (k, K, dV, _, p0, P0), (kr, Kr, dVr, _, p0r, P0r) = out, ref
    m = _ratio((k.double() - kr).abs().amax((0, 2)), kr.abs().amax((0, 2)))
    m = torch.maximum(m, _ratio(((K.double() - Kr).abs() * W).amax(3), (Kr.abs() * W).amax(3)).amax((0, 2)))
    m = torch.maximum(m, _ratio(((P0.double() - P0r).abs() * W).amax(2), (P0r.abs() * W).amax(2)).amax(1))
    m = torch.maximum(m, _ratio(((p0.double() - p0r).abs() * W).amax(1), (p0r.abs() * W).amax(1)))
    return torch.maximum(m, _ratio((dV.double() - dVr).abs(), dVr.abs()).amax(1))


def _floor():
    from oracle.f16_oracle import Oracle
    s, u, act, G, gu = _inputs(256, 4)
    ga, hs, ha = _cost(256, 4)
    o, st, S, U = Oracle('heading'), Oracle.new_state(256), [], []
    st['s'][:], st['u'][:] = s, u
    for a in act:
        S.append(st['s'].copy())
        o.update(st, a)
        U.append(st['u'].copy())
    keep = _kept(np.stack(S), np.stack(U))
    ref = _sweep(torch.float64, S, U, act, G, ga, gu, hs, ha, MU)
    assert (ref[3] == -1).all()
    return 1 - keep.double().mean().item(), _metric(_sweep(torch.float32, S, U, act, G, ga, gu, hs, ha, MU), ref)[keep].max().item()


def _run(b, s, u, act, G, gu, cost, mu=MU, af=F16, edit=None, **kw):
    """fly on the device, sweep on the device and in fp64 about the device's own points -> (device outputs (row-major, cpu), fp64 outputs, kept rows)"""
    ga, hs, ha = cost
    sd, ud, ad = _dev(s.T), _dev(u.T), _dev(act)
    traj = b.rollout(ad, sd, ud, record_every=1)[2]
    U = np.stack([b.rollout(ad[:t + 1], sd, ud)[1].cpu().numpy().T for t in range(len(act))])
    if edit:
        edit(traj)
    S = np.concatenate((s[None], traj[:-1].permute(0, 2, 1).cpu().numpy()))
    k, K, dV, status, p0, P0 = b.ilqr_backward(ad, traj, _dev(G.transpose(0, 2, 1)), _dev(ga.transpose(0, 2, 1)), hs, ha, mu if np.isscalar(mu) else _dev(mu),
                                               g_u_end=_dev(gu[:, :4].T), s=sd, u=ud, want_value=True, **kw)
    out = (k.permute(0, 2, 1).cpu(), K.permute(0, 3, 1, 2).cpu(), dV.t().cpu(), status.cpu(), p0.t().cpu(), P0.permute(2, 0, 1).cpu())
    return out, _sweep(torch.float64, S, U, act, G, ga, gu, hs, ha, mu, af), _kept(S, U)


def test_against_the_fp64_sweep_teacher_forced():
    s, u, act, G, gu = _inputs(256, 4)
    out, ref, keep = _run(_batch(), s, u, act, G, gu, _cost(256, 4))
    assert (ref[3] == -1).all() and (out[3] == -1).all()
    m = _metric(out, ref)[keep]
    print(f'excluded {1 - keep.double().mean().item():.4f}; worst metric on {int(keep.sum())} rows: {m.max().item():.3e} (tol {TOL:.3e})')
    assert 1 - keep.double().mean().item() <= MAX_EXCLUDED and m.max().item() <= TOL
    assert (np.abs(act) > 1).any() and (out[1] != 0).any()


def test_without_a_hessian_it_is_the_reverse_sweep_and_the_batch_is_left_as_it_was():
    """h_s = 0, h_a = 1, mu = 0, no direct action gradient: P stays zero, k_t = -(rollout_vjp's action gradient), p0 = its start gradients"""
    n, H = 65, 3
    s, u, act, G, gu = _inputs(n, H)
    b, twin, sd, ud, ad, Gd = _batch(n), _batch(n), _dev(s.T), _dev(u.T), _dev(act), _dev(G.transpose(0, 2, 1))
    for x in (b, twin):
        x.reset(want_obs=False)
        x.step(ad[0].clamp(-1, 1))   # the cross-step coefficient cache is live from here on
    was = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    traj = b.rollout(ad, sd, ud, record_every=1)[2]
    g_s0, g_u0, g_a = b.rollout_vjp(ad, traj, Gd, _dev(gu.T), s=sd, u=ud)
    k, K, _, status, p0, P0 = b.ilqr_backward(ad, traj, Gd, torch.zeros((H, 4, n), device='cuda'), np.zeros((H, 12), np.float32), np.ones(4, np.float32), 0.0,
                                              g_u_end=_dev(gu[:, :4].T), s=sd, u=ud, want_value=True)
    assert (status == -1).all() and (K == 0).all() and (P0 == 0).all()
    m = _vjp_metric(p0.t().cpu(), -k.permute(0, 2, 1).cpu(), torch.cat((g_s0, g_u0[:4])).t().cpu().double(), g_a.cpu().double())
    assert m.max().item() <= VJP_TOL
    now = b.state_dict()   # a pure function: state, flags, counters; and a disturbed coefficient cache would show in the next step
    assert all(torch.equal(v, now[k]) if torch.is_tensor(v) else v == now[k] for k, v in was.items())
    assert all(torch.equal(x, y) for x, y in zip(b.step(ad[0].clamp(-1, 1)), twin.step(ad[0].clamp(-1, 1)))) and torch.equal(b.s, twin.s)


_BIG = {}


@pytest.mark.parametrize('n,H', [(n, H) for n in (1, 7, 8, 9, 63, 64, 65, 129) for H in (1, 3)])
def test_shapes_and_grids_bit_for_bit(n, H):
    s, u, act, G, gu = _inputs(129, H)
    cost, b = _cost(129, H), _batch()
    if H not in _BIG:   # the larger launch and its fp64 reference, once per horizon
        _BIG[H] = _run(b, s, u, act, G, gu, cost)
    big, ref, keep = _BIG[H]
    for groups in (0, 1):   # the same rows as part of a larger launch, and under one workgroup that walks the tiles
        out = _run(b, s[:n], u[:n], act[:, :n], G[:, :n], gu[:n], (cost[0][:, :n],) + cost[1:], max_groups=groups, ld_out=n + 3)[0]
        assert all(torch.equal(x, y) for x, y in zip(out, _rows_of(big, slice(0, n)))), f'rows depend on their neighbours or the grid (max_groups={groups})'
    assert _metric(big, ref)[keep].max().item() <= TOL


@pytest.mark.parametrize('case', ['all_clamped', 'failed_pivot', 'inf_gradient', 'alpha_nan', 'airframe', 'fanout'])
def test_edge_rows(case):
    n, H = 65, 3
    s, u, act, G, gu = _inputs(n, H)
    cost, mu, edit, kw = _cost(n, H), MU, None, {}
    af = {'mass': 700, 'Jy': 60000} if case == 'airframe' else None
    if case == 'all_clamped':
        act[:, 3] = np.float32([1.5, -1.5, 1.0000001, -2])
    elif case == 'failed_pivot':   # a per-row mu at or below -h_a is the caller's device data: with D = 0, Qt = (h_a + mu) I is not positive
        act[:, 3], mu = 1.5, np.full(n, MU, np.float32)
        mu[3] = -1.5
    elif case == 'inf_gradient':
        G[1, 3, 6] = np.inf
    elif case == 'alpha_nan':
        def edit(traj):
            traj[1, 7, 3] = float('nan')
    b = _batch(airframe=af)
    if case == 'fanout':   # output row r starts from start row r // 3
        src, m = np.arange(63) // 3, slice(0, 63)
        out = _run(b, s[src], u[src], act[:, m], G[:, m], gu[m], (cost[0][:, m],) + cost[1:])[0]   # the same starts, copied out on the host
        sd, ud, ad = _dev(s[:21].T), _dev(u[:21].T), _dev(act[:, m])
        traj = b.rollout(ad, sd, ud, fanout=3, record_every=1)[2]
        fan = b.ilqr_backward(ad, traj, _dev(G[:, m].transpose(0, 2, 1)), _dev(cost[0][:, m].transpose(0, 2, 1)), cost[1], cost[2], MU,
                              g_u_end=_dev(gu[m, :4].T), s=sd, u=ud, fanout=3)
        assert fan[0].shape == (H, 4, 63) and torch.equal(fan[0].permute(0, 2, 1).cpu(), out[0]) and torch.equal(fan[1].permute(0, 3, 1, 2).cpu(), out[1])
        return
    out, ref, keep = _run(b, s, u, act, G, gu, cost, mu=mu, af=dict(F16, **af) if af else F16, edit=edit)
    clean = _run(b, *_inputs(n, H), _cost(n, H))[0] if case in ('failed_pivot', 'inf_gradient', 'alpha_nan') else None
    keep[3] &= case not in ('failed_pivot', 'inf_gradient', 'alpha_nan')
    assert _metric(out, ref)[keep].max().item() <= TOL
    k, K, dV, status, p0, P0 = out
    if case == 'all_clamped':   # D = 0: k = -g_a / (h_a + mu) to the bit, K = 0
        want = -torch.from_numpy(cost[0][:, 3]) / (torch.from_numpy(cost[2]) + torch.tensor(MU, dtype=torch.float32))
        assert torch.equal(k[:, 3], want) and (K[:, 3] == 0).all() and status[3] == -1
    elif case in ('failed_pivot', 'inf_gradient'):
        t = H - 1 if case == 'failed_pivot' else 1
        assert status[3] == t == ref[3][3] and (status[[2, 4]] == -1).all()
        assert (k[:t + 1, 3] == 0).all() and (K[:t + 1, 3] == 0).all() and (dV[3] == 0).all() and (p0[3] == 0).all() and (P0[3] == 0).all()
        assert all(torch.equal(x, y) for x, y in zip(_rows_of(out, [2, 4]), _rows_of(clean, [2, 4])))
        assert case == 'failed_pivot' or (torch.equal(k[2, 3], clean[0][2, 3]) and torch.equal(K[2, 3], clean[1][2, 3]))
    elif case == 'alpha_nan':   # the poisoned point is (s_2, u_3): steps 2 .. 0 are NaN, the neighbours are those of a launch without it
        assert torch.isnan(k[:, 3]).all() and torch.isnan(K[:, 3]).all() and torch.isnan(dV[3]).all() and torch.isnan(P0[3]).all()
        assert all(torch.equal(x, y) for x, y in zip(_rows_of(out, [2, 4]), _rows_of(clean, [2, 4])))
    elif case == 'airframe':
        assert _metric(out, _run(_batch(), s, u, act, G, gu, cost)[1])[keep].max().item() > TOL, 'the airframe must matter, or this compares nothing'


@pytest.mark.parametrize('what,match', [('fleet', 'fleet'), ('gemm', 'aero_gemm_order'), ('tables', 'aero_1d_tables'), ('rk4', 'rk4'), ('combat', 'SingleCombat')])
def test_contexts_without_a_riccati_sweep_are_refused_by_name(what, match):
    from neuralplane_amd.core import F16Batch, F16CombatBatch
    from neuralplane_amd.envs.utils.utils import parse_config
    kw = {'fleet': dict(airframes=[{}, {'mass': 700}]), 'gemm': dict(aero_gemm_order=True), 'tables': dict(aero_1d_tables=True), 'rk4': dict(solver='rk4')}.get(what, {})
    b = F16CombatBatch(4, parse_config('selfplay'), 'cuda:0') if what == 'combat' else _batch(8, **kw)
    z = lambda *shape: torch.zeros(shape, device='cuda')  # noqa: E731
    with pytest.raises(RuntimeError, match=match):
        F16Batch.ilqr_backward(b, z(2, 8, 4), z(2, 12, 8), z(2, 12, 8), z(2, 4, 8), np.zeros((2, 12), np.float32), np.ones(4, np.float32), 0.0, s=z(12, 8), u=z(5, 8))
