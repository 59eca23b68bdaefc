"""np_f16_model_lqr without a GPU: `_lqr_ref`, the restatement of the structured doubling that tests/test_gpu_lqr.py trusts, against scipy's DARE
solver and against the finite-horizon Riccati sweep; the symbol, the record's layout and the checks that run before a launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

DT, LAG_KEEP, GAIN = 0.02, 0.9, (0.1 * 0.225 * 76300.0 / 0.3048, 4.5, 4.5, 4.5)   # F16Model.update's literals
NO_POS_HEADING, LONGITUDINAL = 0xFFFF & ~0b100011, sum(1 << k for k in (2, 4, 6, 7, 10, 12, 13))   # core.LQR_NO_POSITION_HEADING, LQR_LONGITUDINAL
LQR_TOL = 2e-5                               # the call's default tol (core.LQR_TOL)
_KEEP = []


def _equilibration(hs, ha, select):
    """T of np_f16_lqr_io: powers of two from the weights and the control gains, 1 for coordinates without a weight"""
    x = np.ones(16)
    for i in range(12):
        if (select >> i) & 1 and hs[i] > 0:
            x[i] = 1 / math.sqrt(hs[i])
    x[12:] = np.asarray(GAIN) / np.sqrt(np.asarray(ha, np.float64))
    return 2.0 ** np.clip(np.round(np.log2(x)), -40, 40)


def _problem(J, hs, ha, select, dtype, equilibrate=False):
    """(A_d, B_d, Q, R) [n, 16, 16], [n, 16, 4], [16, 16], [4, 4] of include/neuralplane_amd.h (np_f16_lqr_io) from J = [A | B] [n, 12, 16];
    with `equilibrate` in the coordinates x = T x~, and T as the fifth"""
    n, J = J.shape[0], J.to(dtype)
    m = torch.tensor([(select >> k) & 1 for k in range(16)], dtype=dtype)
    Phi = torch.eye(16, dtype=dtype).repeat(n, 1, 1)
    Phi[:, :12] += DT * J
    S = torch.cat((torch.ones(12, dtype=dtype), LAG_KEEP * torch.ones(4, dtype=dtype)))
    Ad = m[:, None] * (Phi * S) * m
    Bd = m[:, None] * Phi[:, :, 12:] * torch.tensor(GAIN, dtype=dtype)
    Q = torch.diag(torch.cat((torch.as_tensor(hs, dtype=dtype), torch.zeros(4, dtype=dtype))) * m)
    R = torch.diag(torch.as_tensor(ha, dtype=dtype))
    if not equilibrate:
        return Ad, Bd, Q, R
    T = torch.as_tensor(_equilibration(hs, ha, select), dtype=dtype)
    return Ad * T / T[:, None], Bd / T[:, None], Q * T * T[:, None], R, T


def _lqr_ref(dtype, J, hs, ha, select=0xFFFF, tol=LQR_TOL, max_doublings=24, equilibrate=True):
    """the doubling of np_f16_lqr_io, term by term, in `dtype` -> K [n, 4, 16], P [n, 16, 16], doublings [n], res [n], status [n] (0 or 1)"""
    Ad, Bd, Q, R, T = _problem(J, hs, ha, select, dtype, True) if equilibrate else _problem(J, hs, ha, select, dtype) + (torch.ones(16, dtype=dtype),)
    n, eye, sym = J.shape[0], torch.eye(16, dtype=dtype), lambda X: 0.5 * (X + X.transpose(1, 2))  # noqa: E731
    A, G, H = Ad, Bd @ torch.linalg.solve(R, Bd.transpose(1, 2)), Q.repeat(n, 1, 1)
    live, doublings, res = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.int32), torch.full((n,), math.inf, dtype=dtype)
    for _ in range(max_doublings):
        XY = torch.linalg.solve(eye + G @ H, torch.cat((A, G), 2))
        X, Y = XY[:, :, :16], XY[:, :, 16:]
        A1, G1, H1 = A @ X, sym(G + A @ Y @ A.transpose(1, 2)), sym(H + A.transpose(1, 2) @ H @ X)
        d = torch.diagonal(H1, dim1=1, dim2=2)
        dd = d[:, :, None] * d[:, None, :]
        crit = torch.where(dd > 0, (H1 - H).abs() / dd.clamp_min(torch.finfo(dtype).tiny).sqrt(), torch.zeros((), dtype=dtype)).amax((1, 2))
        w = live[:, None, None]
        A, G, H = torch.where(w, A1, A), torch.where(w, G1, G), torch.where(w, H1, H)
        res, doublings = torch.where(live, crit, res), doublings + live.int()
        live = live & ~(crit <= tol)
    BtH = Bd.transpose(1, 2) @ H
    return -torch.linalg.solve(R + BtH @ Bd, BtH @ Ad) / T, H / T / T[:, None], doublings, res, live.int()


def _metric(K, P, Kr, Pr):
    """per row, section 17's metric: each output row of K and P in W's units, relative to the reference row's maximum (a zero row must be zero)"""
    from test_gpu_ilqr import _ratio
    from test_gpu_linearize import W
    m = _ratio(((K.double() - Kr).abs() * W).amax(2), (Kr.abs() * W).amax(2)).amax(1)
    return torch.maximum(m, _ratio(((P.double() - Pr).abs() * W).amax(2), (Pr.abs() * W).amax(2)).amax(1))


def _rows(n=130):
    """the GPU test's rows: the fp32-rounded Jacobians of test_gpu_linearize's flight conditions, and the weights of test_gpu_ilqr._cost"""
    from test_gpu_ilqr import _cost
    from test_gpu_linearize import _jac
    if not _KEEP:
        _KEEP.append(_jac(torch.float64)[1].float())
    _, hs, ha = _cost(1, 1)
    return _KEEP[0][:n], hs[0], ha


def _floor(equilibrate=True):
    J, hs, ha = _rows()
    K, P, _, _, st = _lqr_ref(torch.float32, J, hs, ha, NO_POS_HEADING, equilibrate=equilibrate)
    Kr, Pr, _, _, str_ = _lqr_ref(torch.float64, J, hs, ha, NO_POS_HEADING)
    assert (st == 0).all() and (str_ == 0).all()
    return _metric(K, P, Kr, Pr).max().item()


def test_the_restatement_is_the_dare_solution_in_fp64():
    from scipy.linalg import solve_discrete_are
    J, hs, ha = _rows(32)
    K, P, doublings, _, status = _lqr_ref(torch.float64, J, hs, ha, NO_POS_HEADING, tol=1e-13, max_doublings=32)
    Ad, Bd, _, R = _problem(J, hs, ha, NO_POS_HEADING, torch.float64)
    sel = [k for k in range(16) if (NO_POS_HEADING >> k) & 1]
    q = np.diag(np.concatenate((hs, np.zeros(4)))[sel])
    for i in range(32):
        a, b = Ad[i][sel][:, sel].numpy(), Bd[i][sel].numpy()
        p = solve_discrete_are(a, b, q, R.numpy())
        scale = np.sqrt(np.outer(np.diag(p), np.diag(p)))
        assert np.abs(P[i][sel][:, sel].numpy() - p).max() <= 1e-9 * np.abs(p).max() and (np.abs(P[i][sel][:, sel].numpy() - p) / scale).max() <= 1e-7
        k = -np.linalg.solve(R.numpy() + b.T @ p @ b, b.T @ p @ a)
        assert np.abs(K[i][:, sel].numpy() - k).max() <= 1e-7 * np.abs(k).max()
    rest = [k for k in range(16) if k not in sel]
    assert (status == 0).all() and doublings.max() <= 24 and (K[:, :, rest] == 0).all() and (P[:, rest] == 0).all() and (P[:, :, rest] == 0).all()


def test_three_doublings_are_eight_steps_of_the_riccati_sweep():
    """H after j doublings is the P that step 0 of a 2^j-step sweep of np_f16_ilqr_io consumes (the sweep adds the stage cost before a step,
    the DARE after it), and the gain is that step's"""
    from test_gpu_ilqr import _riccati
    J, hs, ha = _rows(32)
    f64, n = torch.float64, 32
    K, H, doublings, _, _ = _lqr_ref(f64, J, hs, ha, tol=1e-300, max_doublings=3)
    Phi = torch.eye(16, dtype=f64).repeat(n, 1, 1)
    Phi[:, :12] += DT * J.double()

    def sweep(steps):
        z = lambda *s: torch.zeros(s, dtype=f64)  # noqa: E731
        return _riccati(Phi.repeat(steps, 1, 1, 1), torch.tensor(GAIN, dtype=f64).repeat(steps, n, 1), z(steps, n, 12), z(steps, n, 4), z(n, 4),
                        torch.from_numpy(hs).double().repeat(steps, 1), torch.from_numpy(ha).double(), z(n), LAG_KEEP)
    Q = torch.diag(torch.cat((torch.from_numpy(hs).double(), torch.zeros(4, dtype=f64))))
    assert (doublings == 3).all()
    assert torch.allclose(sweep(8)[1][0], K, rtol=1e-9, atol=0) and torch.allclose(sweep(7)[5] + Q, H, rtol=1e-9, atol=1e-12 * H.abs().max().item())


def test_the_gpu_tests_floor_is_what_the_cpu_recipe_gives():
    """TOL_FP32_SELF of tests/test_gpu_lqr.py is `_floor()`; a CPU's fp32 LAPACK varies with its build, so the literal is reproduced within a factor 2"""
    import test_gpu_lqr as g
    floor = _floor()
    print(floor)
    assert g.TOL_FP32_SELF / 2 <= floor <= g.TOL_FP32_SELF * 2


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16LqrIo()
    io.A = io.B = io.K = io.doublings = io.res = io.status = 64   # never dereferenced: the call is refused on the host
    io.ld, io.ld_out, io.select, io.max_doublings, io.tol = 8, 8, 0xFFFF, 24, 1e-5
    io.h_s, io.h_a = (C.c_float * 12)(*[1.0] * 12), (C.c_float * 4)(*[1.0] * 4)
    return io


def test_symbol_and_record_layout(lib):
    from neuralplane_amd import _lib
    assert 'np_f16_model_lqr' in _lib.EXPORTS and lib.np_f16_model_lqr is not None and lib.np_abi_version() == _lib.ABI_VERSION == 16
    R = _lib.NpF16LqrIo
    assert C.sizeof(R) == 160   # the values the header's static_asserts state (include/neuralplane_amd.h)
    want = {'ld': 16, 'K': 24, 'doublings': 40, 'ld_out': 64, 'select': 72, 'max_doublings': 76, 'tol': 88, 'h_s': 92, 'h_a': 140}
    assert {k: getattr(R, k).offset for k in want} == want


@pytest.mark.parametrize('field,value,n,match', [
    (('h_s', 3), -1.0, 8, b'h_s'), (('h_s', 11), math.nan, 8, b'h_s'), (('h_a', 0), 0.0, 8, b'h_a'), (('h_a', 3), math.inf, 8, b'h_a'), ('tol', 0.0, 8, b'tol'),
    ('tol', math.nan, 8, b'tol'), ('max_doublings', -1, 8, b'max_doublings'), ('max_doublings', 33, 8, b'max_doublings'), ('select', 1 << 16, 8, b'select'),
    ('A', None, 8, b'null input'), ('B', None, 8, b'null input'), ('K', None, 8, b'null output'), ('doublings', None, 8, b'null output'), ('res', None, 8, b'null output'),
    ('status', None, 8, b'null output'), ('ld', 7, 8, b'ld must'), ('ld', 1 << 30, 8, b'ld must'), ('ld_out', 7, 8, b'ld_out'), ('max_groups', -1, 8, b'max_groups'),
    ('reserved_', 1, 8, b'reserved_'), ('ld', 8, 0, b'n must be')])
def test_validation_runs_on_the_host_before_any_launch(lib, field, value, n, match):
    """every refusal of the record comes before the context is looked at: a null context reaches it"""
    io = _valid_io()
    if isinstance(field, tuple):
        getattr(io, field[0])[field[1]] = value
    else:
        setattr(io, field, value)
    assert lib.np_f16_model_lqr(None, n, C.byref(io), None) != 0 and match in lib.np_last_error(), lib.np_last_error()
    assert lib.np_f16_model_lqr(None, n, None, None) != 0 and b'null io' in lib.np_last_error()


def test_a_valid_record_stops_at_the_null_context(lib):
    io = _valid_io()
    for p in (None, 64):   # without and with the optional P
        io.P = p
        assert lib.np_f16_model_lqr(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()
