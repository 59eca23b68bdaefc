"""The host side of np_f16_model_rollout_feedback without a GPU (the symbol and the checks that run before a launch), and the fp64
restatement of the law that tests/test_gpu_ilqr_forward.py trusts: one backward sweep plus this forward law is the exact LQR minimiser."""
import ctypes as C

import numpy as np
import pytest
import torch

_KEEP = []   # host arrays the records point into


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16FeedbackIo()
    for k in ('s0', 'u0', 'actions', 's_traj', 'k', 'K', 'actions_out', 's_out', 'u_out', 's_traj_out', 'ws', 'cost', 'best', 's_ref'):
        setattr(io, k, 64)   # never dereferenced: the call is refused on the host
    io.ld0, io.ld, io.ld_out, io.act_row_stride, io.act_step_stride, io.traj_step_stride, io.horizon, io.fanout, io.n_alpha = 8, 8, 16, 4, 32, 96, 2, 1, 2
    _KEEP.extend((np.float32([1, 0.5, 0.25]), np.ones((2, 12), np.float32)))
    io.alphas, io.h_s, io.h_a = _KEEP[-2].ctypes.data, _KEEP[-1].ctypes.data, (C.c_float * 4)(1, 1, 1, 1)
    return io


@pytest.mark.parametrize('field,value,match', [
    ('K', None, b'null gains'), ('alphas', None, b'alphas'), ('s_init', 64, b's_init and u_init'), ('s_traj_out', None, b'null output'), ('ws', None, b'ws'),
    ('cost', None, b'best needs cost'), ('h_s', None, b'cost needs h_s'), ('n_alpha', 3, b'power of two'), ('n_alpha', 65, b'n_alpha must be in [1, 64]'),
    ('n_alpha', 0, b'n_alpha'), ('alphas[1]', 1.5, b'alphas must be finite and in [0, 1]'), ('alphas[1]', float('nan'), b'alphas must be finite'),
    ('h_s[1, 7]', -1e-6, b'h_s must be finite and not negative'), ('h_a', (C.c_float * 4)(1, -1, 1, 1), b'h_a must be finite'), ('ld', 7, b'ld must'),
    ('ld_out', 15, b'ld_out'), ('act_step_stride', 0, b'act_step_stride'), ('traj_step_stride', 95, b'traj_step_stride'), ('horizon', 0, b'horizon'),
    ('shape', 0, b'null ctx')])
def test_every_refusal_of_the_record_comes_before_a_device_is_touched(field, value, match):
    """a null context reaches every one of them, and np_last_error names the field"""
    from neuralplane_amd import _lib
    lib, io = _lib.load(), _valid_io()
    if field == 'alphas[1]':   # alphas and h_s are host memory and are read by the checks
        _KEEP[-2][1] = value
    elif field == 'h_s[1, 7]':
        _KEEP[-1][1, 7] = value
    else:
        setattr(io, field, value)
    assert 'np_f16_model_rollout_feedback' in _lib.EXPORTS and lib.np_f16_model_rollout_feedback(None, 8, C.byref(io), None) != 0 and match in lib.np_last_error()


def test_one_sweep_and_the_law_at_alpha_one_is_the_lqr_minimiser():
    """H = 3, a random stable Phi per step, no clamp, the fused cost's model about a nominal flight that is not optimal: `_riccati`'s gains flown
    through `_law` and `_lag` (x = (s, u entering the step), kappa inside K) land on the minimiser of the stacked quadratic, from xbar_0 and
    from a perturbed x_0"""
    from test_gpu_ilqr import _riccati
    from test_gpu_ilqr_forward import _lag, _law
    r, H, f64, kappa = np.random.RandomState(6), 3, torch.float64, 0.9
    T = lambda x: torch.from_numpy(np.asarray(x)).to(f64)  # noqa: E731
    Phi, D = T(np.eye(16) * 0.9 + 0.1 * r.standard_normal((H, 16, 16))), T(r.uniform(0.5, 2, (H, 4)))
    hs, ha, ref, abar, xb0 = T(r.uniform(0.5, 1.5, (H, 12))), T(r.uniform(0.5, 1.5, 4)), T(r.standard_normal((H, 12))), T(r.standard_normal((H, 4))), T(r.standard_normal(16))

    def fly(act, x0):   # act(t, x) -> a_t;  u' = kappa u + D a, (s, u')+ = Phi (s, u');  -> (cost, the states x_0..x_{H-1}, the actions)
        x, cost, xs, acts = x0, 0.0, [], []
        for t in range(H):
            xs.append(x)
            acts.append(act(t, x))
            x = Phi[t] @ torch.cat((x[:12], _lag(x[12:, None], acts[-1][:, None], D[t], kappa)[:, 0]))
            cost = cost + 0.5 * (hs[t] * (x[:12] - ref[t]) ** 2).sum() + 0.5 * (ha * acts[-1] ** 2).sum()
        return cost, xs + [x], torch.stack(acts)

    _, xbar, _ = fly(lambda t, x: abar[t], xb0)
    G, ga = torch.stack([hs[t] * (xbar[t + 1][:12] - ref[t]) for t in range(H)]), ha * abar
    k, K, _, status = _riccati(Phi[:, None], D[:, None], G[:, None], ga[:, None], torch.zeros((1, 4), dtype=f64), hs, ha, torch.zeros(1, dtype=f64), kappa)[:4]
    assert status[0] == -1
    one = torch.ones((), dtype=f64)
    for x0 in (xb0, xb0 + 0.1 * T(r.standard_normal(16))):
        flown = fly(lambda t, x: _law(abar[t][:, None], one, k[t, 0][:, None], K[t, 0][:, :, None], x[:, None], xbar[t][:, None])[0][:, 0], x0)[2]
        open_loop = lambda a: fly(lambda t, x: a[t], x0)[0]  # noqa: E731
        z = torch.zeros((H, 4), dtype=f64)
        g = torch.autograd.functional.jacobian(open_loop, z).reshape(-1)
        Hm = torch.autograd.functional.hessian(open_loop, z).reshape(H * 4, H * 4)
        assert torch.allclose(flown, -torch.linalg.solve(Hm, g).reshape(H, 4), rtol=1e-9, atol=1e-9)   # quadratic: one Newton step from zero
