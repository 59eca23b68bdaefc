"""The host side of np_f16_model_mppi without a GPU: the symbol, the record's layout as include/neuralplane_amd.h asserts it, and the checks
that run before a launch."""
import ctypes as C

import numpy as np
import pytest

_KEEP = []   # host arrays the records point into


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16MppiIo()
    for k in ('s0', 'u0', 'actions', 's_ref', 'cost', 'plan_out', 'best', 'ess', 'actions_out', 'ws'):
        setattr(io, k, 64)   # never dereferenced: the call is refused on the host
    io.ld0, io.ld, io.act_row_stride, io.act_step_stride, io.horizon, io.candidates, io.hold, io.temperature = 8, 8, 4, 32, 2, 48, 1, 0.5
    _KEEP.append(np.ones((2, 12), np.float32))
    io.h_s, io.h_a, io.sigma = _KEEP[-1].ctypes.data, (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0.3, 0.3, 0, 0.3)
    return io


def test_the_symbol_and_the_record_are_what_the_header_pins():
    from neuralplane_amd import _lib
    io, off = _lib.NpF16MppiIo, lambda k: getattr(_lib.NpF16MppiIo, k).offset  # noqa: E731
    assert 'np_f16_model_mppi' in _lib.EXPORTS and hasattr(_lib.load(), 'np_f16_model_mppi') and _lib.load().np_abi_version() == 16
    assert C.sizeof(io) == 192 and [off(k) for k in ('actions', 'horizon', 'seed', 'sigma', 'temperature', 'h_s', 'ld', 'h_a', 'cost', 'best', 'actions_out', 'ws')] == \
        [24, 48, 64, 80, 96, 104, 120, 128, 144, 160, 176, 184]


@pytest.mark.parametrize('field,value,match', [
    ('candidates', 0, b'candidates (K) must be in [1, 4096]'), ('candidates', 4097, b'candidates (K)'), ('hold', 0, b'hold must be'),
    ('sigma', (C.c_float * 4)(0.3, -0.1, 0.3, 0.3), b'sigma must be finite and not negative'), ('sigma', (C.c_float * 4)(0.3, 0.3, float('inf'), 0.3), b'sigma'),
    ('temperature', 0.0, b'temperature must be finite and positive'), ('temperature', float('nan'), b'temperature'), ('temperature', float('inf'), b'temperature'),
    ('h_s', None, b'h_s'), ('h_s[1, 7]', -1e-6, b'h_s must be finite and not negative'), ('h_a', (C.c_float * 4)(1, float('nan'), 1, 1), b'h_a must be finite'),
    ('cost', None, b'null cost'), ('s_ref', None, b's_ref'), ('ws', None, b'ws'), ('plan_out', None, b'plan_out'), ('ld', 7, b'ld must'),
    ('act_step_stride', 0, b'act_step_stride'), ('horizon', 0, b'horizon'), ('reserved_', 1, b'reserved_'), ('shape', 0, b'null ctx')])
def test_every_refusal_of_the_record_comes_before_a_device_is_touched(field, value, match):
    """a null context reaches every one of them, and np_last_error names the field"""
    from neuralplane_amd import _lib
    lib, io = _lib.load(), _valid_io()
    if field == 'h_s[1, 7]':   # h_s is host memory and is read by the checks
        _KEEP[-1][1, 7] = value
    else:
        setattr(io, field, value)
    assert lib.np_f16_model_mppi(None, 8, C.byref(io), None) != 0 and match in lib.np_last_error()
