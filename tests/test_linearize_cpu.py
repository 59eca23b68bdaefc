"""The host side of np_f16_model_linearize without a GPU: the symbol, the record's layout, the grid rule and the checks that run before a launch."""
import ctypes as C

import pytest


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16LinearizeIo()
    io.s0 = io.u0 = io.xdot = io.A = io.B = 64   # never dereferenced: the call is refused on the host
    io.ld0, io.ld_out = 8, 8
    return io


def test_symbol_and_record_layout(lib):
    from neuralplane_amd import _lib
    assert lib.np_f16_model_linearize is not None and lib.np_abi_version() == 16
    R = _lib.NpF16LinearizeIo
    # the values the header's static_asserts state (include/neuralplane_amd.h)
    assert C.sizeof(R) == 64
    want = {'ld0': 16, 'xdot': 24, 'B': 40, 'ld_out': 48, 'max_groups': 56}
    assert {k: getattr(R, k).offset for k in want} == want


@pytest.mark.parametrize('n,cus,max_groups,want', [
    (1, 256, 0, 1), (64, 256, 0, 1), (65, 256, 0, 2), (64 * 256, 256, 0, 256), (64 * 256 + 1, 256, 0, 256), (10 ** 6, 256, 0, 256),   # one workgroup per CU at the most
    (10 ** 6, 32, 0, 32), (321, 256, 1, 1), (321, 256, 2, 2), (321, 256, 100, 6),                                                    # the cap is per CU, or the caller's
    (0, 256, 0, None), (1 << 30, 256, 0, None), (100, 0, 0, None), (100, 256, -1, None)])
def test_grid_rule(n, cus, max_groups, want):
    from neuralplane_amd import _lib
    if want is None:
        with pytest.raises(RuntimeError):
            _lib.linearize_groups(n, cus, max_groups)
    else:
        assert _lib.linearize_groups(n, cus, max_groups) == want


@pytest.mark.parametrize('field,value,n,match', [('s0', None, 8, b'null flight condition'), ('u0', None, 8, b'null flight condition'), ('A', None, 8, b'null output'),
                                                 ('B', None, 8, b'null output'), ('ld0', 7, 8, b'ld0'), ('ld_out', 7, 8, b'ld_out'), ('ld_out', 1 << 30, 8, b'ld_out'),
                                                 ('max_groups', -1, 8, b'max_groups'), ('reserved_', 1, 8, b'reserved_'), ('ld0', 8, 0, b'n must be'),
                                                 ('ld0', 1 << 31, 1 << 30, b'n must be')])
def test_validation_runs_on_the_host_before_any_launch(lib, field, value, n, match):
    """every refusal of the record comes before the context is looked at: a null context reaches it"""
    io = _valid_io()
    setattr(io, field, value)
    assert lib.np_f16_model_linearize(None, n, C.byref(io), None) != 0 and match in lib.np_last_error()
    assert lib.np_f16_model_linearize(None, n, None, None) != 0 and b'null io' in lib.np_last_error()


def test_a_valid_record_stops_at_the_null_context(lib):
    io = _valid_io()
    assert lib.np_f16_model_linearize(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()
    io.xdot = None   # xdot is optional
    assert lib.np_f16_model_linearize(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()
