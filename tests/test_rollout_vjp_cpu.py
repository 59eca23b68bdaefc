"""The host side of np_f16_model_rollout_vjp without a GPU: the symbol, the record's layout against the header, and the checks that run before a launch."""
import ctypes as C
import os
import subprocess

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'neuralplane_amd.h')


@pytest.fixture(scope='module')
def lib():
    from neuralplane_amd import _lib
    return _lib.load()


def _valid_io():
    from neuralplane_amd import _lib
    io = _lib.NpF16RolloutVjpIo()
    for k in ('s0', 'u0', 'actions', 's_traj', 'g_s_traj', 'g_s0', 'g_u0', 'g_actions', 'u_ws'):
        setattr(io, k, 64)   # never dereferenced: the call is refused on the host
    io.ld0, io.ld, io.ld_out, io.act_row_stride, io.act_step_stride, io.traj_step_stride, io.horizon, io.fanout = 8, 8, 8, 4, 32, 96, 2, 1
    return io


def test_symbol_is_exported_and_the_record_matches_the_header(lib, tmp_path):
    from neuralplane_amd import _lib
    assert 'np_f16_model_rollout_vjp' in _lib.EXPORTS and lib.np_f16_model_rollout_vjp is not None and lib.np_abi_version() == 16
    R = _lib.NpF16RolloutVjpIo
    names = [k for k, _ in R._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu\\n", sizeof(np_f16_rollout_vjp_io));%s return 0;}' % (
        HEADER, ''.join(f'printf("%zu\\n", offsetof(np_f16_rollout_vjp_io, {k}));' for k in names))
    (tmp_path / 'layout.c').write_text(prog)
    subprocess.run(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(R)] + [getattr(R, k).offset for k in names]


@pytest.mark.parametrize('field,value,n0,match', [
    ('s0', None, 8, b'null start state'), ('u0', None, 8, b'null start state'), ('actions', None, 8, b'null actions'), ('s_traj', None, 8, b's_traj'),
    ('g_s_traj', None, 8, b'g_s_traj'), ('g_s0', None, 8, b'null output'), ('g_u0', None, 8, b'null output'), ('g_actions', None, 8, b'null output'),
    ('u_ws', None, 8, b'u_ws'), ('horizon', 0, 8, b'horizon'), ('fanout', 0, 8, b'fanout'), ('fanout', 1 << 30, 8, b'2^30'), ('ld0', 7, 8, b'ld0'),
    ('ld', 7, 8, b'ld must'), ('ld', 1 << 30, 8, b'ld must'), ('ld_out', 7, 8, b'ld_out'), ('act_row_stride', 3, 8, b'act_row_stride'),
    ('act_step_stride', 31, 8, b'act_step_stride'), ('traj_step_stride', 95, 8, b'traj_step_stride'), ('max_groups', -1, 8, b'max_groups'),
    ('reserved_', 1, 8, b'reserved_'), ('ld0', 8, 0, b'n0 must'), ('ld0', 1 << 31, 1 << 30, b'2^30')])
def test_every_refusal_of_the_record_comes_before_a_device_is_touched(lib, field, value, n0, match):
    """a null context reaches every one of them, and np_last_error names the field"""
    io = _valid_io()
    setattr(io, field, value)
    assert lib.np_f16_model_rollout_vjp(None, n0, C.byref(io), None) != 0 and match in lib.np_last_error()


def test_null_io_and_null_context(lib):
    assert lib.np_f16_model_rollout_vjp(None, 8, None, None) != 0 and b'null io' in lib.np_last_error()
    io = _valid_io()
    assert lib.np_f16_model_rollout_vjp(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()
    io.g_u_end, io.act_step_stride = None, 0   # the controls' cotangent is optional; a held action
    assert lib.np_f16_model_rollout_vjp(None, 8, C.byref(io), None) != 0 and b'null ctx' in lib.np_last_error()


def test_the_gpu_tests_floor_and_exclusion_are_what_the_cpu_recipe_gives():
    """TOL_FP32_SELF of tests/test_gpu_rollout_vjp.py is its `_floor()` (the fp32 recursion against its fp64 self on the oracle's trajectory); the
    fp32 sums of a CPU's BLAS vary with its threads, so the literal is reproduced within a factor 2, the excluded fraction (fp64) exactly"""
    import test_gpu_rollout_vjp as g
    excluded, floor = g._floor()
    assert excluded <= g.MAX_EXCLUDED and abs(excluded - 0.152) < 1e-3 and g.TOL_FP32_SELF / 2 <= floor <= g.TOL_FP32_SELF * 2
