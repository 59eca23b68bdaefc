"""The host side of np_f16_model_trim without a GPU: the symbol, the record's layout and the checks that run before a launch."""
import ctypes as C
import math

import pytest


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16TrimIo()
    io.s0 = io.u0 = io.s = io.u = io.res = io.iters = io.status = 64   # never dereferenced: the call is refused on the host
    io.ld0, io.ld_out, io.m, io.max_iters, io.tol = 8, 8, 3, 20, 1e-3
    for j, (row, z) in enumerate(((6, 7), (7, 12), (10, 13))):
        io.rows[j] = row
        io.D[z][j] = 1.0
    for k in range(12):
        io.scale[k] = 1.0
    for e in range(16):
        io.lo[e], io.hi[e] = -math.inf, math.inf
    return io


def test_symbol_and_record_layout(lib):
    from neuralplane_amd import _lib
    assert 'np_f16_model_trim' in _lib.EXPORTS and lib.np_f16_model_trim is not None and lib.np_abi_version() == 16
    R = _lib.NpF16TrimIo
    # the values the header's static_asserts state (include/neuralplane_amd.h)
    assert C.sizeof(R) == 1128
    want = {'ld0': 24, 's': 32, 'xdot': 80, 'ld_out': 104, 'm': 112, 'tol': 128, 'rows': 136, 'D': 184, 'scale': 952, 'lo': 1000, 'hi': 1064}
    assert {k: getattr(R, k).offset for k in want} == want


def _set(io, field, value):
    if isinstance(field, tuple):   # an element of an array field: (name, index...) 
        arr = getattr(io, field[0])
        for k in field[1:-1]:
            arr = arr[k]
        arr[field[-1]] = value
    else:
        setattr(io, field, value)


@pytest.mark.parametrize('field,value,n,match', [
    ('m', 0, 8, b'm must be'), ('m', 13, 8, b'm must be'), (('rows', 1), 6, 8, b'distinct'), (('rows', 2), 12, 8, b'rows 0..11'), (('rows', 0), -1, 8, b'rows 0..11'),
    (('D', 12, 1), 0.0, 8, b'all zero'), (('lo', 12), 1.0, 8, b'lo must not exceed hi'), ('tol', 0.0, 8, b'tol'), ('tol', math.nan, 8, b'tol'),
    (('scale', 3), 0.0, 8, b'scale'), (('scale', 11), -1.0, 8, b'scale'), ('max_iters', -1, 8, b'max_iters'), ('max_iters', 65, 8, b'max_iters'),
    ('s0', None, 8, b'null start'), ('u0', None, 8, b'null start'), ('s', None, 8, b'null output (s, u)'), ('u', None, 8, b'null output (s, u)'),
    ('res', None, 8, b'res, iters, status'), ('iters', None, 8, b'res, iters, status'), ('status', None, 8, b'res, iters, status'),
    ('A', 64, 8, b'A and B come together'), ('ld0', 7, 8, b'ld0'), ('ld_out', 7, 8, b'ld_out'), ('ld0', 1 << 30, 8, b'ld0'), ('ld_out', 1 << 30, 8, b'ld_out'),
    ('max_groups', -1, 8, b'max_groups'), ('reserved_', 1, 8, b'reserved_'), ('ld0', 8, 0, b'n must be')])
def test_validation_runs_on_the_host_before_any_launch(lib, field, value, n, match):
    """every refusal of the record comes before the context is looked at: a null context reaches it"""
    io = _valid_io()
    if field == ('lo', 12):
        io.hi[12] = 0.0
    _set(io, field, value)
    assert lib.np_f16_model_trim(None, n, C.byref(io), None) != 0 and match in lib.np_last_error(), lib.np_last_error()
    assert lib.np_f16_model_trim(None, n, None, None) != 0 and b'null io' in lib.np_last_error()


def test_a_valid_record_stops_at_the_null_context(lib):
    io = _valid_io()
    assert lib.np_f16_model_trim(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()
    for names in (('xdot',), ('A', 'B'), ('backtracks',)):   # each optional output on its own: xdot alone, then A and B beside it, then the counter
        for k in names:
            setattr(io, k, 64)
        assert lib.np_f16_model_trim(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()


@pytest.mark.parametrize('kind,m', [('longitudinal', 3), ('six_dof', 6), ('turn', 10)])
def test_trim_problem(kind, m):
    from neuralplane_amd.core import trim_problem
    D, rows, scale, lo, hi = trim_problem(kind)
    assert tuple(D.shape) == (16, m) and len(set(rows)) == m and len(scale) == 12 and (D.abs().sum(0) > 0).all()
    assert lo[12] == 0.0 and hi[12] == pytest.approx(0.225 * 76300 / 0.3048) and hi[13:] == [-x for x in lo[13:]] and all(math.isinf(x) for x in lo[:12])
    assert (D[4, 0] == 1.0 and D[7, 0] == 1.0) == (kind != 'turn')   # theta follows alpha where the flight-path angle is held
