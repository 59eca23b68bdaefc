"""The host side of np_f16_model_ilqr_backward without a GPU (the symbol and the checks that run before a launch), and the
fp64 restatement of the sweep that tests/test_gpu_ilqr.py trusts, against the exact LQR solution of a small linear system."""
import ctypes as C

import numpy as np
import pytest
import torch

_KEEP = []   # host arrays the records point into


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def _valid_io(h_s=None):
    from neuralplane_amd import _lib
    io = _lib.NpF16IlqrIo()
    for k in ('s0', 'u0', 'actions', 's_traj', 'g_s_traj', 'g_actions_in', 'k', 'K', 'dV', 'status', 'u_ws', 'p_ws', 'h_ws'):
        setattr(io, k, 64)   # never dereferenced: the call is refused on the host
    io.ld0, io.ld, io.ld_out, io.act_row_stride, io.act_step_stride, io.traj_step_stride, io.horizon, io.fanout = 8, 8, 8, 4, 32, 96, 2, 1
    _KEEP.append(np.ascontiguousarray(np.ones((2, 12)) if h_s is None else h_s, np.float32))
    io.h_s, io.h_a, io.mu = _KEEP[-1].ctypes.data, (C.c_float * 4)(1, 1, 1, 1), 1e-3
    return io


@pytest.mark.parametrize('field,value,n0,match', [
    ('s0', None, 8, b'null start state'), ('actions', None, 8, b'null actions'), ('g_s_traj', None, 8, b'g_s_traj'), ('g_actions_in', None, 8, b'g_actions_in'),
    ('h_s', None, 8, b'h_s'), ('K', None, 8, b'null output'), ('status', None, 8, b'null output'), ('p0', 64, 8, b'p0 and P0'), ('p_ws', None, 8, b'p_ws'),
    ('h_ws', None, 8, b'h_ws'), ('horizon', 0, 8, b'horizon'), ('fanout', 0, 8, b'fanout'), ('ld0', 7, 8, b'ld0'), ('ld', 7, 8, b'ld must'),
    ('ld_out', 7, 8, b'ld_out'), ('act_row_stride', 3, 8, b'act_row_stride'), ('act_step_stride', 0, 8, b'act_step_stride'),
    ('traj_step_stride', 95, 8, b'traj_step_stride'), ('max_groups', -1, 8, b'max_groups'), ('mu', -1.0, 8, b'h_a[k] + mu'), ('mu', float('nan'), 8, b'mu must be finite'),
    ('h_a', (C.c_float * 4)(1, 1, -1, 1), 8, b'h_a[k] + mu'), ('h_a', (C.c_float * 4)(1, float('inf'), 1, 1), 8, b'h_a[k] + mu'), ('ld0', 8, 0, b'n0 must'),
    ('h_s[1, 7]', -1e-6, 8, b'h_s must be finite and not negative'), ('h_s[1, 7]', float('nan'), 8, b'h_s must be finite'), ('h_s[1, 7]', 0.0, 8, b'null ctx')])
def test_every_refusal_of_the_record_comes_before_a_device_is_touched(lib, field, value, n0, match):
    """a null context reaches every one of them, and np_last_error names the field"""
    from neuralplane_amd import _lib
    io = _valid_io()
    if field.startswith('h_s['):   # h_s is host memory and is read by the checks; zero is legal, and a valid record stops at the null context
        _KEEP[-1][1, 7] = value
    else:
        setattr(io, field, value)
    assert 'np_f16_model_ilqr_backward' in _lib.EXPORTS and lib.np_f16_model_ilqr_backward(None, n0, C.byref(io), None) != 0 and match in lib.np_last_error()


def test_the_fp64_restatement_is_the_lqr_solution():
    """H = 3, a random stable Phi per step, no clamp: the gains of `_riccati` (mu = 0) against the minimiser of the stacked quadratic, from x_0 = 0
    and from a random x_0, and (p0, P0, dV) against the optimal cost"""
    from test_gpu_ilqr import _riccati
    r, H, f64 = np.random.RandomState(4), 3, torch.float64
    T = lambda x: torch.from_numpy(np.asarray(x)).to(f64)  # noqa: E731
    Phi = T(np.eye(16) * 0.9 + 0.1 * r.standard_normal((H, 1, 16, 16)))
    D, G, ga, gu = T(r.uniform(0.5, 2, (H, 1, 4))), T(r.standard_normal((H, 1, 12))), T(r.standard_normal((H, 1, 4))), T(r.standard_normal((1, 4)))
    hs, ha, kappa = T(r.uniform(0.5, 1.5, (H, 12))), T(r.uniform(0.5, 1.5, 4)), 0.9
    k, K, dV, status, p0, P0 = _riccati(Phi, D, G, ga, gu, hs, ha, torch.zeros(1, dtype=f64), kappa)
    assert status[0] == -1

    def fly(a, x0):   # x = (s, u): u' = kappa u + D a, (s, u')+ = Phi (s, u'); the cost on s_1..s_H, a_0..a_{H-1} and u_H
        x, cost = x0, 0.0
        for t in range(H):
            x = Phi[t, 0] @ torch.cat((x[:12], kappa * x[12:] + D[t, 0] * a[t]))
            cost = cost + G[t, 0] @ x[:12] + 0.5 * (hs[t] * x[:12] ** 2).sum() + ga[t, 0] @ a[t] + 0.5 * (ha * a[t] ** 2).sum()
        return cost + gu[0] @ x[12:]

    def closed_loop(x0):
        x, acts = x0, []
        for t in range(H):
            acts.append(k[t, 0] + K[t, 0] @ x)
            x = Phi[t, 0] @ torch.cat((x[:12], kappa * x[12:] + D[t, 0] * acts[-1]))
        return torch.stack(acts)
    for x0 in (torch.zeros(16, dtype=f64), T(r.standard_normal(16))):
        z = torch.zeros((H, 4), dtype=f64)
        g = torch.autograd.functional.jacobian(lambda a: fly(a, x0), z).reshape(-1)
        Hm = torch.autograd.functional.hessian(lambda a: fly(a, x0), z).reshape(H * 4, H * 4)
        best = -torch.linalg.solve(Hm, g).reshape(H, 4)   # the cost is quadratic: one Newton step from zero is its minimiser
        assert torch.allclose(closed_loop(x0), best, rtol=1e-9, atol=1e-9)
        want = fly(best, x0) - fly(z, torch.zeros(16, dtype=f64))
        assert torch.allclose(dV[0].sum() + p0[0] @ x0 + 0.5 * x0 @ P0[0] @ x0, want, rtol=1e-9, atol=1e-9)


def test_the_gpu_tests_floor_and_exclusion_are_what_the_cpu_recipe_gives():
    """TOL_FP32_SELF of tests/test_gpu_ilqr.py is its `_floor()` (the fp32 sweep against its fp64 self on the oracle's trajectory); the fp32 sums of
    a CPU's BLAS vary with its threads, so the literal is reproduced within a factor 2, the excluded fraction (fp64) exactly"""
    import test_gpu_ilqr as g
    excluded, floor = g._floor()
    print(excluded, floor)
    assert excluded <= g.MAX_EXCLUDED and abs(excluded - 0.152) < 1e-3 and g.TOL_FP32_SELF / 2 <= floor <= g.TOL_FP32_SELF * 2
