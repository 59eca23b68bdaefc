"""np_f16_model_ekf without a GPU: `_ekf_ref`, the restatement of the filter that tests/test_gpu_ekf.py trusts, against the textbook Kalman
filter on a linear system; the GPU test's inputs, floors and exclusion; the symbol, the record's size and the checks that run before a launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_gpu_linearize import F16, _jac, _nlplant, _load_nets  # noqa: E402
from test_gpu_linearize import _rows as _flight_rows  # noqa: E402
from test_gpu_rollout_vjp import DT, GAIN, LAG_KEEP, MAX_EXCLUDED, _kept  # noqa: E402

SENSORS = sum(1 << k for k in (2, 3, 4, 5, 6, 9, 10, 11))   # alt, the attitude, vt and the body rates
# 1-sigma magnitudes of x = (s[12], u[0:4]), the units of the means' error: a tenth of test_gpu_linearize.W, ten feet for the position
SCALE = np.array([10, 10, 100, 0.01, 0.01, 0.01, 1, 0.001, 0.001, 0.01, 0.01, 0.01, 100, 0.1, 0.1, 0.1])
_CACHE = {}


def _f16_model(dtype):
    def model(s, up):
        return _jac(dtype, s.numpy(), torch.cat((up, torch.zeros_like(up[:, :1])), 1).numpy(), F16)
    return model


def _ekf_ref(dtype, s, u, P0, act, z, q, r, measure, scale=None, model=None):
    """np_f16_ekf_io's definition, term by term, in `dtype`: s [n, 12], u [n, >=4], P0 [n, 16, 16], act [H, n, 4], z [H, n, 16] (NaN = missing),
    q, r [16]; scale [16] or None: the equilibration x = T x~ that np_f16_ekf_io keeps a field for -> x [H, n, 16], P [H, n, 16, 16] (the posteriors), nis [H, n], and the linearisation points (S [H, n, 12], U [H, n, 5]).
    model(s, u') -> (xdot [n, 12], [A | B] [n, 12, 16]); default: the autograd Jacobian of test_gpu_linearize's restatement of nlplant."""
    tt = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)  # noqa: E731
    model = model or _f16_model(dtype)
    x, P, act, z, q, n = torch.cat((tt(s), tt(u)[:, :4]), 1), tt(P0), tt(act), tt(z), tt(q), 1 / tt(r)
    T = tt(2.0 ** np.clip(np.round(np.log2(np.ones(16) if scale is None else scale)), -40, 40))
    bits = torch.tensor([(measure >> k) & 1 == 1 for k in range(16)])
    eye, sym, Sg = torch.eye(16, dtype=dtype), lambda X: 0.5 * (X + X.transpose(1, 2)), torch.cat((torch.ones(12), LAG_KEEP * torch.ones(4))).to(dtype)  # noqa: E731
    Pt, xs, Ps, nis, S, U = P / T / T[:, None], [], [], [], [], []
    for a, zt in zip(act, z):
        up = LAG_KEEP * x[:, 12:] + GAIN.to(dtype) * a.clamp(-1, 1)
        S.append(x[:, :12].double().numpy()), U.append(torch.cat((up, torch.zeros_like(up[:, :1])), 1).double().numpy())
        xd, J = model(x[:, :12], up)
        xm = torch.cat((x[:, :12] + DT * xd, up), 1)
        Phi = eye.repeat(len(x), 1, 1)
        Phi[:, :12] += DT * J
        F = (Phi * Sg) * T / T[:, None]
        Pm = sym(F @ Pt @ F.transpose(1, 2)) + torch.diag(q / T / T)
        seen = bits & torch.isfinite(zt)
        zt = torch.where(seen, zt, torch.zeros_like(zt))
        nt, nu = torch.where(seen, n * T * T, torch.zeros_like(zt)), torch.where(seen, zt - xm, torch.zeros_like(zt))
        Pp = sym(torch.linalg.solve(eye + Pm * nt[:, None, :], Pm))
        Pt = torch.where(seen.any(1)[:, None, None], Pp, Pm)
        x = xm + T * torch.einsum('nij,nj->ni', Pt, nt * (nu / T))
        nis.append((torch.where(seen, n, torch.zeros_like(zt)) * nu * (zt - x)).sum(1))
        xs.append(x), Ps.append(Pt * T * T[:, None])
    return torch.stack(xs), torch.stack(Ps), torch.stack(nis), (np.stack(S), np.stack(U))


def _metric(x, P, nis, xr, Pr, nisr):
    """[3, rows]: the means' error in SCALE units, |dP_ij| / sqrt(P_ii P_jj) and |d nis| / (1 + nis), each at its worst entry"""
    d = torch.diagonal(Pr, dim1=-2, dim2=-1)
    return torch.stack((((x.double() - xr).abs() / torch.from_numpy(SCALE)).amax(-1), ((P.double() - Pr).abs() / (d[..., None] * d[..., None, :]).sqrt()).amax((-2, -1)),
                        (nis.double() - nisr).abs() / (1 + nisr.abs())))


def _inputs(n=130, H=3):
    """the GPU test's rows: test_gpu_linearize's flight conditions as the prior mean, P0 = SCALE (random SPD, condition <= 1e3) SCALE, random
    actions, and z = the fp64 flight from the prior mean plus noise of variance r, on all 16 coordinates"""
    if 'in' not in _CACHE:
        rs, (s, u) = np.random.RandomState(23), _flight_rows()
        s, u = s[:130], u[:130]
        Qm = np.linalg.qr(rs.standard_normal((130, 16, 16)))[0]
        P0 = SCALE[:, None] * (Qm * 10.0 ** rs.uniform(-2, 1, (130, 1, 16)) @ Qm.transpose(0, 2, 1)) * SCALE
        act = rs.uniform(-1.2, 1.2, (3, 130, 4)).astype(np.float32)   # beyond +-1: some are clamped
        q, r = ((0.05 * SCALE) ** 2).astype(np.float32), ((0.5 * SCALE) ** 2).astype(np.float32)
        recs, x, z = _load_nets(), torch.from_numpy(np.hstack((s, u[:, :4]))).double(), []
        for a in torch.from_numpy(act).double():
            up = LAG_KEEP * x[:, 12:] + GAIN * a.clamp(-1, 1)
            x = torch.cat((x[:, :12] + DT * _nlplant(recs, x[:, :12], up), up), 1)
            z.append(x.numpy() + np.sqrt(r) * rs.standard_normal((130, 16)))
        _CACHE['in'] = (s, u, (0.5 * (P0 + P0.transpose(0, 2, 1))).astype(np.float32), act, np.stack(z).astype(np.float32), q, r)
    s, u, P0, act, z, q, r = _CACHE['in']
    return s[:n], u[:n], P0[:n], act[:H, :n], z[:H, :n], q, r


def _reference(measure):
    """the fp64 restatement on the 130 rows over three steps, and the rows it keeps away from a ReLU kink; once per sensor set"""
    if measure not in _CACHE:
        out = _ekf_ref(torch.float64, *_inputs(), measure)
        _CACHE[measure] = out[:3] + (_kept(*out[3]),)
    return _CACHE[measure]


def _floor(measure, equilibrate=True):
    """(excluded fraction, the worst kept row of each component of `_metric` over the three steps) of the fp32 restatement against its fp64 self"""
    xr, Pr, nisr, keep = _reference(measure)
    x, P, nis, _ = _ekf_ref(torch.float32, *_inputs(), measure, SCALE if equilibrate else None)
    return 1 - keep.double().mean().item(), _metric(x, P, nis, xr, Pr, nisr)[:, :, keep].amax((1, 2)).tolist()


def test_the_restatement_is_the_textbook_filter_on_a_linear_system():
    """a random stable linear plant behind the lag: K = P C^T (C P C^T + R)^-1, the Joseph update and NIS = nu^T S^-1 nu, in fp64"""
    rs, n, H, f64 = np.random.RandomState(7), 4, 5, torch.float64
    A, B = torch.from_numpy(-2 * np.eye(12) + rs.standard_normal((12, 12))), torch.from_numpy(rs.standard_normal((12, 4)))
    J = torch.cat((A, B), 1).repeat(n, 1, 1)
    s, u, act = rs.standard_normal((n, 12)), rs.standard_normal((n, 4)), rs.uniform(-1.2, 1.2, (H, n, 4))
    M = rs.standard_normal((n, 16, 16))
    P0, q, r = M @ M.transpose(0, 2, 1) + np.eye(16), rs.uniform(0.01, 0.1, 16), rs.uniform(0.1, 1, 16)
    z = rs.standard_normal((H, n, 16))
    z[2, 1, 4], z[3] = np.nan, np.nan   # one sample missing, one step without any
    xs, Ps, nis, _ = _ekf_ref(f64, s, u, P0, act, z, q, r, SENSORS, rs.uniform(0.01, 100, 16), lambda s_, up: (s_ @ A.T + up @ B.T, J))
    x, P, idx = torch.from_numpy(np.hstack((s, u))), torch.from_numpy(P0), [k for k in range(16) if (SENSORS >> k) & 1]
    Phi = torch.eye(16, dtype=f64)
    Phi[:12] += DT * J[0]
    F = Phi * torch.cat((torch.ones(12), LAG_KEEP * torch.ones(4))).double()
    for t in range(H):
        for i in range(n):
            up = LAG_KEEP * x[i, 12:] + GAIN * torch.from_numpy(act[t, i]).clamp(-1, 1)
            xm, Pm = torch.cat((x[i, :12] + DT * (A @ x[i, :12] + B @ up), up)), F @ P[i] @ F.T + torch.diag(torch.from_numpy(q))
            seen = [k for k in idx if np.isfinite(z[t, i, k])]
            if not seen:
                x[i], P[i] = xm, Pm
                assert nis[t, i] == 0
                continue
            Cm, R = torch.eye(16, dtype=f64)[seen], torch.diag(torch.from_numpy(r[seen]))
            nu, Sm = torch.from_numpy(z[t, i, seen]) - Cm @ xm, Cm @ Pm @ Cm.T + R
            K = Pm @ Cm.T @ torch.linalg.inv(Sm)
            x[i], IKC, want = xm + K @ nu, torch.eye(16, dtype=f64) - K @ Cm, (nu @ torch.linalg.solve(Sm, nu)).item()
            P[i] = IKC @ Pm @ IKC.T + K @ R @ K.T
            assert abs(nis[t, i].item() - want) <= 1e-9 * (1 + want)
        assert torch.allclose(xs[t], x, rtol=1e-9, atol=1e-9 * x.abs().max().item()) and torch.allclose(Ps[t], P, rtol=1e-9, atol=1e-9 * P.abs().max().item())


@pytest.mark.parametrize('measure', [SENSORS, 0, 0xFFFF])
def test_the_gpu_tests_floors_and_exclusion_are_what_the_cpu_recipe_gives(measure):
    """FLOOR of tests/test_gpu_ekf.py is `_floor()`; a CPU's fp32 LAPACK varies with its build, so the literals are reproduced within a factor 2,
    and the reference alone keeps the excluded rows within the cap.  Without the equilibration the covariance's floor is more than twice as high:
    the reason np_f16_ekf_io keeps it"""
    import test_gpu_ekf as g
    excluded, floor = _floor(measure)
    print(excluded, floor)
    assert excluded <= MAX_EXCLUDED and all(lit / 2 <= f <= lit * 2 for lit, f in zip(g.FLOOR[measure], floor) if lit > 0) and len(floor) == 3
    if measure == SENSORS:
        assert _floor(measure, equilibrate=False)[1][1] > 2 * floor[1]


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16EkfIo()
    for k in ('s0', 'u0', 'P0', 'z', 'actions', 's_out', 'u_out', 'P_out', 'status', 'p_ws'):
        setattr(io, k, 64)   # never dereferenced: the call is refused on the host
    io.ld0, io.ld, io.ld_out, io.act_row_stride, io.act_step_stride, io.horizon, io.measure = 8, 8, 8, 4, 32, 2, SENSORS
    io.q, io.r, io.scale = ((C.c_float * 16)(*[1.0] * 16) for _ in range(3))
    return io


def test_symbol_and_record_size(lib):
    from neuralplane_amd import _lib
    assert 'np_f16_model_ekf' in _lib.EXPORTS and lib.np_f16_model_ekf is not None and lib.np_abi_version() == _lib.ABI_VERSION == 16
    assert C.sizeof(_lib.NpF16EkfIo) == 352   # the header's static_assert (include/neuralplane_amd.h)


@pytest.mark.parametrize('field,value,n,match', [
    (('q', 3), -1.0, 8, b'q must'), (('q', 15), math.nan, 8, b'q must'), (('r', 2), 0.0, 8, b'r must'), (('r', 11), math.inf, 8, b'r must'), (('r', 0), 0.0, 8, b'null ctx'),
    (('scale', 5), 0.0, 8, b'scale'), (('scale', 5), math.nan, 8, b'scale'), ('horizon', 0, 8, b'horizon'), ('measure', 1 << 16, 8, b'measure'), ('measure', -1, 8, b'measure'),
    ('s0', None, 8, b'null prior'), ('P0', None, 8, b'null prior'), ('actions', None, 8, b'null actions'), ('z', None, 8, b'null measurements'),
    ('P_out', None, 8, b'null output'), ('status', None, 8, b'null output'), ('p_ws', None, 8, b'p_ws'), ('ld0', 7, 8, b'ld0'), ('ld', 7, 8, b'ld must'),
    ('ld', 1 << 30, 8, b'ld must'), ('ld_out', 7, 8, b'ld_out'), ('act_row_stride', 3, 8, b'act_row_stride'), ('act_step_stride', 31, 8, b'act_step_stride'),
    ('act_step_stride', 0, 8, b'null ctx'), ('max_groups', -1, 8, b'max_groups'), ('reserved_', 1, 8, b'reserved_'), ('ld', 8, 0, b'n must be')])
def test_every_refusal_of_the_record_comes_before_a_device_is_touched(lib, field, value, n, match):
    """a null context reaches every one of them, and np_last_error names the field; an unmeasured r and a held action are legal"""
    io = _valid_io()
    if isinstance(field, tuple):
        getattr(io, field[0])[field[1]] = value
    else:
        setattr(io, field, value)
    assert lib.np_f16_model_ekf(None, n, C.byref(io), None) != 0 and match in lib.np_last_error(), lib.np_last_error()
    assert lib.np_f16_model_ekf(None, n, None, None) != 0 and b'null io' in lib.np_last_error()
