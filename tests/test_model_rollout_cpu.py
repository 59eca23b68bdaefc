"""The host side of np_f16_model_rollout without a GPU: the symbol, the record's layout, the shape rule and the checks that run before a launch."""
import ctypes as C

import pytest


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def test_symbol_and_record_layout(lib):
    from neuralplane_amd import _lib
    assert lib.np_f16_model_rollout is not None and lib.np_abi_version() == 16
    R = _lib.NpF16RolloutIo
    # the values the header's static_asserts state (include/neuralplane_amd.h)
    assert C.sizeof(R) == 104
    want = {'actions': 24, 'horizon': 48, 'shape': 60, 's_out': 64, 'ld_out': 80, 'traj_step_stride': 96}
    assert {k: getattr(R, k).offset for k in want} == want


@pytest.mark.parametrize('rows,cus,solver,pin,want', [
    (1, 256, 0, 'auto', 'split'), (64 * 256, 256, 0, 'auto', 'split'), (64 * 256 + 1, 256, 0, 'auto', 'throughput'), (10 ** 6, 256, 0, 'auto', 'throughput'),
    (64 * 32, 32, 0, 'auto', 'split'), (64 * 32 + 1, 32, 0, 'auto', 'throughput'),                 # the threshold is per CU
    (1, 256, 1, 'auto', 'throughput'), (3000, 256, 1, 'auto', 'throughput'),                         # rk4 is never split
    (10 ** 6, 256, 0, 'split', 'split'), (1, 256, 0, 'throughput', 'throughput'), (1, 256, 1, 'throughput', 'throughput'),   # a pin is honoured ...
    (3000, 256, 1, 'split', None), (0, 256, 0, 'auto', None), (100, 0, 0, 'auto', None), (100, 256, 0, 3, None)])           # ... or refused
def test_shape_rule(rows, cus, solver, pin, want):
    from neuralplane_amd import _lib
    if want is None:
        with pytest.raises(RuntimeError):
            _lib.rollout_shape(rows, cus, solver, pin)
    else:
        assert _lib.rollout_shape(rows, cus, solver, pin) == want


@pytest.mark.parametrize('field,value,match', [('s0', None, b'null start state'), ('actions', None, b'null actions'), ('u_out', None, b'null output'),
                                               ('horizon', 0, b'horizon'), ('fanout', 0, b'fanout'), ('record_every', -1, b'record_every'),
                                               ('s_traj', 64, b's_traj without record_every'), ('act_row_stride', 3, b'act_row_stride'), ('ld_out', 7, b'ld_out')])
def test_validation_runs_on_the_host_before_any_launch(lib, field, value, match):
    """every refusal of the record comes before the context is looked at: a null context reaches it"""
    from neuralplane_amd import _lib
    io = _lib.NpF16RolloutIo()
    io.s0 = io.u0 = io.actions = io.s_out = io.u_out = 64   # never dereferenced: the call is refused on the host
    io.ld0, io.ld_out, io.act_row_stride, io.act_step_stride, io.horizon, io.fanout = 8, 8, 4, 32, 2, 1
    setattr(io, field, value)
    assert lib.np_f16_model_rollout(None, 8, C.byref(io), None) != 0 and match in lib.np_last_error()
    assert lib.np_f16_model_rollout(None, 8, None, None) != 0 and b'null io' in lib.np_last_error()


def test_a_valid_record_stops_at_the_null_context(lib):
    from neuralplane_amd import _lib
    io = _lib.NpF16RolloutIo()
    io.s0 = io.u0 = io.actions = io.s_out = io.u_out = 64
    io.ld0, io.ld_out, io.act_row_stride, io.act_step_stride, io.horizon, io.fanout = 8, 8, 4, 32, 2, 1
    assert lib.np_f16_model_rollout(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()
