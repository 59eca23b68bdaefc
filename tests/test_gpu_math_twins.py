"""The device's elementary functions against the oracle's, bit for bit (np_selfcheck_math == f16o_math_array): sincos_d / np_sincos /
np_sincostan, log2_d / exp2_d / np_pow / np_pow_posexp, np_acos, np_atanh, np_exp, np_norm3, np_dot3, np_wrap_pi (csrc/np_math.h) and the
controller's act_exp / act_sigmoid / act_tanh (csrc/np_actor.h), on the all-binade grid and each function's edge list
(tests/math_spec.py) — the branches no trajectory reaches: the fmod path of |x| >= 2^30, quadrants at multiples of pi/2 +- ulps, ldexp
into fp32 / fp64 denormals and at the +-2000 clamp, the sqrt(2) seam of the logarithm, acos beyond +-1, atanh at +-1, the special-value
ladders of pow, act_exp at its clamps, rintf ties and NaN, the denormal quotient of act_sigmoid(-inf).  What the oracle's functions
are worth against truth is tests/test_math_spec_cpu.py's subject.

What this pins is the functions as the library's flags compile them into the self-check kernel (the same inline functions, no copies;
csrc/ holds no other restatement of these sequences).  Their inlined instances inside the big kernels stay covered by the trajectory
tests.  Every test also asserts that each named edge class of its function contributed rows (classified on the host from the input
values), and writes its counts to math_selfcheck.json in the report directory.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import math_spec as ms  # noqa: E402
from oracle import f16_oracle as fo  # noqa: E402  (the checker; test infrastructure)
from test_gpu_edge_cases import _write_report  # noqa: E402

F32 = np.float32
REPORT = {}


def _device(fn, x, param=0.0):
    from neuralplane_amd import _lib
    lib = _lib.load()
    ci, co = fo.MATH_COLS[fn]
    x = np.ascontiguousarray(x, F32).reshape(-1, ci)
    out = np.empty((x.shape[0], co), F32)
    _lib.check(lib.np_selfcheck_math(fo.MATH_FN[fn], x.shape[0], x.ctypes.data, ci, C.c_double(param), out.ctypes.data, co, 0))
    return out


@pytest.mark.parametrize('fn', list(fo.MATH_FN))
def test_device_equals_oracle_bit_for_bit(fn):
    inputs, mismatches, hits, first = 0, 0, {}, None
    for x, param in ms.batches(fn):
        assert x.shape[0] <= ms.MAX_ROWS
        got, want = _device(fn, x, param), fo.math_array(fn, x, param)
        bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(1)
        # -0 == +0 is not forgiven: the comparison is on the bits, NaN == NaN apart
        inputs += x.shape[0]
        mismatches += int(np.count_nonzero(bad))
        if bad.any() and first is None:
            i = int(np.nonzero(bad)[0][0])
            first = {'input': x[i].tolist(), 'param': param, 'device': got[i].tolist(), 'oracle': want[i].tolist()}
        for k, m in ms.classes(fn, x, param).items():
            hits[k] = hits.get(k, 0) + int(np.count_nonzero(m))
    REPORT[fn] = {'inputs': inputs, 'mismatches': mismatches, 'first_mismatch': first, 'rows_per_edge_class': hits}
    _write_report('math_selfcheck.json', REPORT)
    assert mismatches == 0, (fn, mismatches, first)
    assert all(v > 0 for v in hits.values()), (fn, [k for k, v in hits.items() if v == 0])


def test_argument_checks():
    from neuralplane_amd import _lib
    lib = _lib.load()
    x, o = np.zeros(64, F32), np.full(64, 7, F32)
    call = lambda fn, n, xi, ci, p, oo, co, dev=0: lib.np_selfcheck_math(fn, n, xi, ci, C.c_double(p), oo, co, dev)   # noqa: E731
    X, O = x.ctypes.data, o.ctypes.data
    assert call(0, 4, X, 1, 0.0, O, 2) == 0 and (o[:8].reshape(4, 2) == [0, 1]).all() and (o[8:] == 7).all()      # writes n rows and nothing behind them
    assert call(0, 0, X, 1, 0.0, O, 2) == 0                                                                          # nothing to do
    for bad, word in (((13, 4, X, 1, 0.0, O, 1), b'unknown'), ((-1, 4, X, 1, 0.0, O, 1), b'unknown'), ((0, 4, X, 2, 0.0, O, 2), b'columns'),
                      ((0, 4, X, 1, 0.0, O, 1), b'columns'), ((8, 4, X, 3, 0.0, O, 1), b'columns'), ((0, 4, None, 1, 0.0, O, 2), b'null'),
                      ((0, 4, X, 1, 0.0, None, 2), b'null'), ((4, (1 << 24) + 1, X, 1, 0.0, O, 1), b'2^24'), ((4, -1, X, 1, 0.0, O, 1), b'2^24'),
                      ((3, 4, X, 1, 0.0, O, 1), b'positive'), ((3, 4, X, 1, float('nan'), O, 1), b'positive'), ((0, 4, X, 1, 0.0, O, 2, 99), b'device')):
        assert call(*bad) != 0 and word in lib.np_last_error(), (bad, lib.np_last_error())
    assert (o[8:] == 7).all()
