"""What the oracle's elementary functions are worth against truth (CPU; their device twins are held to them bit for bit by
tests/test_gpu_math_twins.py).  The inputs are those of tests/math_spec.py — the all-binade grid and the edge lists — restricted to
each function's mathematical domain.

Stage one compares with numpy's fp64 libm rounded to fp32: at most 1 input in 1 000 may differ (the project's own bound; it only
limits the cost of stage two and forgives nothing).  Stage two adjudicates every differing input, and every edge-list value
regardless, with mpmath at 160 bits: |oracle - truth| <= (0.5 + 2^-10) ulp32, which holds only while the fp64 sequence's relative
error stays below 2^-34.  Where the spec defines something other than the plain function, truth is that definition, also in mpmath:
sin / cos of fmod(x, fp64(2 pi)) for |x| >= 2^30, the dot product of fp32-rounded products.  The measured excess over 0.5 ulp32 goes
to math_spec_cpu.json (report directory).  The controller's fp32 exp / sigmoid / tanh have no analytic bound: they are measured
against fp64 libm and asserted at twice the measured value (constants in math_spec.py).
"""
import ctypes as C
import math
import os
import re

import mpmath
import numpy as np
import pytest

import math_spec as ms
from oracle import f16_oracle as fo

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP = mpmath.mp.clone()
MP.prec = 160
BOUND = 0.5 + 2.0 ** -10
REPORT = {}


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _report(name, **kw):
    """The measured figures, through the suite's report writer (the module that holds it needs no GPU to import)."""
    from test_gpu_edge_cases import _write_report
    REPORT.setdefault(name, {}).update(kw)
    _write_report('math_spec_cpu.json', REPORT)


def _ulp_error(o, t):
    """|o - t| in ulp32 of the truth t (an mpmath number); the oracle's infinity counts as 2^128, results below 2^-126 use the denormal spacing."""
    o = float(o)
    if t == 0:
        return abs(o) / 2.0 ** -149
    if abs(t) >= MP.mpf(2) ** 128:
        return 0.0 if (math.isinf(o) and (o > 0) == (t > 0)) else float('inf')
    if math.isinf(o):
        o = math.copysign(2.0 ** 128, o)
    if math.isnan(o):
        return float('inf')
    e = max(MP.mag(t) - 1, -126)
    return float(abs(MP.mpf(o) - t) / MP.mpf(2) ** (e - 23))


def _adjudicate(name, x, got, truth_row, idx):
    """Stage two over the rows `idx`: the largest error in ulp32 per output column, asserted against the bound."""
    worst, at = 0.0, None
    for i in idx:
        t = truth_row(x[i])
        for j, tj in enumerate(t):
            err = _ulp_error(got[i, j], tj)
            if err > worst:
                worst, at = err, (x[i].tolist(), j, float(got[i, j]))
    _report(name, adjudicated=int(len(idx)), max_error_ulp32=worst, excess_over_half_ulp32=max(worst - 0.5, 0.0), at=at)
    assert worst <= BOUND, (name, worst, at)
    return worst


def _two_stages(name, fn, x, ref64, truth_row, param=0.0, n_edge=0):
    """x [n, in_cols]: the rows in the function's domain, the last n_edge of them from the edge list.  ref64: fp64 libm reference [n, out_cols]."""
    got = fo.math_array(fn, x, param)
    with np.errstate(all='ignore'):
        ref = np.asarray(ref64, np.float64).astype(F32).reshape(got.shape)
    same = _same(got, ref).all(1)
    frac = float(np.mean(same))
    _report(name, inputs=int(x.shape[0]), differ_from_fp64_libm=int(np.count_nonzero(~same)))
    assert frac > 0.999, (name, frac)
    idx = np.union1d(np.nonzero(~same)[0], np.arange(x.shape[0] - n_edge, x.shape[0]))
    return _adjudicate(name, x, got, truth_row, idx)


def _domain(fn, keep):
    """(rows of all batches of fn for which keep(x) holds, number of trailing edge-list rows among them); one param only."""
    x = ms.batches(fn)[0][0]
    g = x[:x.shape[0] - ms.edges(fn).shape[0]]
    e = np.unique(ms.edges(fn), axis=0)
    with np.errstate(all='ignore'):
        g, e = g[keep(g)], e[keep(e)]
    return np.concatenate([g, e]), e.shape[0]


# ---- ids ---------------------------------------------------------------------------------------------------------------------------
def test_function_ids_and_columns_are_the_same_on_both_sides():
    """NP_MATH_* of the public header == F16O_MATH_* of the oracle's header == the Python table; f16o_math_array refuses what np_selfcheck_math refuses."""
    for path, prefix in ((os.path.join(ROOT, 'include', 'neuralplane_amd.h'), 'NP_MATH_'), (os.path.join(ROOT, 'oracle', 'f16_oracle.h'), 'F16O_MATH_')):
        ids = {k: int(v) for k, v in re.findall(prefix + r'([A-Z0-9_]+) = (\d+)', open(path).read())}
        assert ids.pop('NUM_FN') == len(fo.MATH_FN) and ids == fo.MATH_FN, path
    assert set(fo.MATH_COLS) == set(fo.MATH_FN) == set(ms._EDGES)
    lib = C.CDLL(fo.build())
    lib.f16o_math_array.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int]
    x, o = np.zeros(8, F32), np.zeros(8, F32)
    assert lib.f16o_math_array(0, 1, x.ctypes.data, 1, 0.0, o.ctypes.data, 2) == 0
    for bad in ((13, 1, 1, 1), (-1, 1, 1, 1), (0, 1, 1, 1), (0, 1, 2, 2), (8, 1, 3, 1), (0, -1, 1, 2)):
        assert lib.f16o_math_array(bad[0], bad[1], x.ctypes.data, bad[2], 0.0, o.ctypes.data, bad[3]) != 0, bad
    assert lib.f16o_math_array(0, 1, None, 1, 0.0, o.ctypes.data, 2) != 0
    for fn in fo.MATH_FN:                                                       # the batched entry is the scalar functions the old tests call
        e = ms.edges(fn)[:50]
        assert fo.math_array(fn, e, ms.ATM_EXP).shape == (e.shape[0], fo.MATH_COLS[fn][1])
    o = fo.Oracle('heading')
    e = ms.edges('POW')[::7]
    assert _same(fo.math_array('POW', e)[:, 0], [o.pow(a, b)[0] for a, b in e]).all()
    assert _same(fo.math_array('POW_POSEXP', e[:, :1], ms.ATM_EXP)[:, 0], o.pow(e[:, 0], 4.14)).all()   # np_pow_posexp == np_pow(x, (float)y)


def test_the_grid_is_what_the_spec_says():
    g = ms.grid()
    b = g.view(np.uint32)
    assert g.size == 2 * 256 * (16 + 2 ** 13) and np.unique(b).size == g.size
    per = np.bincount((b >> 23).astype(np.int64), minlength=512)
    assert (per == 16 + 2 ** 13).all()                                          # every sign x exponent field equally
    assert np.isnan(g).sum() == 2 * (16 + 2 ** 13) - 2 and np.isinf(g).sum() == 2 and (g == 0).sum() == 2
    for fn in fo.MATH_FN:
        zero = [k for k, v in ms.class_counts(fn).items() if v == 0]
        assert not zero, (fn, zero)


# ---- fp64 sequences against truth -----------------------------------------------------------------------------------------------
def _sincos_truth(row):
    x = float(row[0])
    if not abs(x) < 2.0 ** 30:
        x = math.fmod(x, ms.TWO_PI_D)                                           # the spec's definition for |x| >= 2^30 (exact remainder)
    c, s = MP.cos_sin(MP.mpf(x))
    return s, c, (s / c)


def test_sincos_and_tan_against_truth():
    x, n_edge = _domain('SINCOSTAN', lambda v: np.isfinite(v[:, 0]))
    xd = x[:, 0].astype(np.float64)
    xr = np.where(np.abs(xd) < 2.0 ** 30, xd, np.fmod(xd, ms.TWO_PI_D))
    _two_stages('sincostan', 'SINCOSTAN', x, np.stack([np.sin(xr), np.cos(xr), np.tan(xr)], 1), _sincos_truth, n_edge=n_edge)
    assert _same(fo.math_array('SINCOS', x), fo.math_array('SINCOSTAN', x)[:, :2]).all()


def _pow_domain(v):
    return np.isfinite(v).all(1) & (v[:, 0] > 0)


def test_pow_against_truth():
    worst = 0.0
    for b, (xb, _) in enumerate(ms.batches('POW')):
        n_e = ms.edges('POW').shape[0] if b == 0 else 0
        g = xb[:xb.shape[0] - n_e]
        e = np.unique(ms.edges('POW'), axis=0) if b == 0 else xb[:0]
        with np.errstate(all='ignore'):
            g, e = g[_pow_domain(g)], e[_pow_domain(e)]
        if g.shape[0] == 0:
            continue
        x = np.concatenate([g, e])
        with np.errstate(all='ignore'):
            ref = np.power(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64))
        worst = max(worst, _two_stages(f'pow_y{b}', 'POW', x, ref, lambda r: (MP.power(MP.mpf(float(r[0])), MP.mpf(float(r[1]))),), n_edge=e.shape[0]))
    assert worst > 0


@pytest.mark.parametrize('param', ms.POSEXP_PARAMS)
def test_pow_posexp_against_truth(param):
    x, n_edge = _domain('POW_POSEXP', lambda v: np.isfinite(v[:, 0]) & (v[:, 0] > 0))
    with np.errstate(all='ignore'):
        ref = np.power(x[:, 0].astype(np.float64), param)
    _two_stages(f'pow_posexp_{param!r}', 'POW_POSEXP', x, ref, lambda r: (MP.power(MP.mpf(float(r[0])), MP.mpf(param)),), param=param, n_edge=n_edge)


def test_acos_against_truth():
    x, n_edge = _domain('ACOS', lambda v: np.abs(v[:, 0]) <= 1)
    _two_stages('acos', 'ACOS', x, np.arccos(x[:, 0].astype(np.float64)), lambda r: (MP.acos(MP.mpf(float(r[0]))),), n_edge=n_edge)


def test_exp_against_truth():
    x, n_edge = _domain('EXP', lambda v: np.isfinite(v[:, 0]))
    with np.errstate(all='ignore'):
        ref = np.exp(x[:, 0].astype(np.float64))
    _two_stages('exp', 'EXP', x, ref, lambda r: (MP.exp(MP.mpf(float(r[0]))),), n_edge=n_edge)


def test_atanh_against_truth_on_the_rewards_arguments_and_in_absolute_terms_elsewhere():
    """np_atanh = ln((1 + x) / (1 - x)) / 2 cancels near 0 by construction.  On the arguments its call site can produce
    (math_spec.atanh_reachable: multiples of 2^-24 in [-0.9, 1 - 1e-4]) it meets the ulp condition, zero included; elsewhere in (-1, 1) the
    error is bounded in absolute terms only: 2^-51 from the three roundings of the quotient and the fp64 logarithm, plus the final rounding.
    Measured outside the reachable set: see math_spec_cpu.json (the relative error reaches 100 % where 1 + x rounds to 1)."""
    x, n_edge = _domain('ATANH', lambda v: ms.atanh_reachable(v[:, 0]))
    _two_stages('atanh_reachable', 'ATANH', x, np.arctanh(x[:, 0].astype(np.float64)), lambda r: (MP.atanh(MP.mpf(float(r[0]))),), n_edge=n_edge)
    x, _ = _domain('ATANH', lambda v: np.abs(v[:, 0]) < 1)
    got = fo.math_array('ATANH', x)[:, 0].astype(np.float64)
    t = np.arctanh(x[:, 0].astype(np.float64))
    err = np.abs(got - t)
    with np.errstate(all='ignore'):
        ulp = ms.ulp32(t.astype(F32))
        rel = np.where(t != 0, err / np.abs(t), 0)
    i = int(np.argmax(err / ulp))
    _report('atanh_open_interval', inputs=int(x.shape[0]), max_abs_error=float(err.max()), max_error_ulp32=float((err / ulp).max()), at=float(x[i, 0]),
            max_rel_error=float(rel.max()))
    assert (err <= 2.0 ** -51 + (BOUND + 2.0 ** -20) * ulp).all(), float((err - BOUND * ulp).max())


def test_norm3_and_dot3_against_truth():
    fin = lambda v: np.isfinite(v).all(1)                                       # noqa: E731
    for b in range(2):
        xb = ms.batches('NORM3')[b][0]
        n_e = ms.edges('NORM3').shape[0] if b == 0 else 0
        g, e = xb[:xb.shape[0] - n_e], np.unique(xb[xb.shape[0] - n_e:], axis=0)
        x = np.concatenate([g[fin(g)], e[fin(e)]])
        d = x.astype(np.float64)
        _two_stages(f'norm3_{b}', 'NORM3', x, np.sqrt((d * d).sum(1)), lambda r: (MP.sqrt(sum(MP.mpf(float(v)) ** 2 for v in r)),), n_edge=int(fin(e).sum()))
    for b in range(2):
        xb = ms.batches('DOT3')[b][0]
        n_e = ms.edges('DOT3').shape[0] if b == 0 else 0
        with np.errstate(all='ignore'):
            ok = lambda v: fin(v) & np.isfinite((v[:, :3] * v[:, 3:]).astype(F32)).all(1)   # noqa: E731  (finite fp32 products: the rest is a special value)
            g, e = xb[:xb.shape[0] - n_e], np.unique(xb[xb.shape[0] - n_e:], axis=0)
            x = np.concatenate([g[ok(g)], e[ok(e)]])
            p = (x[:, :3] * x[:, 3:]).astype(F32).astype(np.float64)            # the spec rounds each product to fp32 first
            n_edge = int(ok(e).sum())

        def truth(r):
            with np.errstate(all='ignore'):
                q = (r[:3] * r[3:]).astype(F32)
            return (sum(MP.mpf(float(v)) for v in q),)
        _two_stages(f'dot3_{b}', 'DOT3', x, (p[:, 0] + p[:, 1]) + p[:, 2], truth, n_edge=n_edge)


def test_wrap_pi_is_the_written_definition():
    """np_wrap_pi has no rounding freedom: torch.remainder (exact fmod, + divisor on a sign mismatch), then the two fp32 corrections — restated in
    numpy fp32, whose fmod is exact, it must agree bit for bit on the grid and the edge list; the result lies in [-pi_f, pi_f]."""
    x = ms.batches('WRAP_PI')[0][0][:, 0]
    got = fo.math_array('WRAP_PI', x)[:, 0]
    with np.errstate(all='ignore'):
        r = np.fmod(x, ms.TWO_PI_F)
        r = np.where((r != 0) & (r < 0), r + ms.TWO_PI_F, r)
        r = r + np.where(r < 0, ms.TWO_PI_F, F32(0))
        r = (r - np.where(r > ms.PI_F, ms.TWO_PI_F, F32(0))).astype(F32)
    assert r.dtype == F32 and _same(got, r).all()
    fin = np.isfinite(x)
    assert np.isnan(got[~fin]).all() and (np.abs(got[fin]) <= ms.PI_F).all()
    d = (got[fin].astype(np.float64) - x[fin].astype(np.float64)) / np.float64(ms.TWO_PI_F)       # a whole number of fp32(2 pi) away, up to the two roundings
    small = np.abs(x[fin]) < 1e4
    assert np.abs(d[small] - np.rint(d[small])).max() < 1e-6


# ---- special values, from the ladders of the code ------------------------------------------------------------------------------------
INF, NAN = np.inf, np.nan
PI32, PIO2_32 = float(F32(np.pi)), float(F32(np.pi / 2))
SPECIAL = {
    'SINCOS': [((INF,), (NAN, NAN)), ((-INF,), (NAN, NAN)), ((NAN,), (NAN, NAN)), ((0.0,), (0, 1)), ((-0.0,), (0, 1))],
    'SINCOSTAN': [((INF,), (NAN, NAN, NAN)), ((NAN,), (NAN, NAN, NAN)), ((0.0,), (0, 1, 0))],
    # np_pow tests NaN first, then the sign of the base, then zero and infinite bases by the sign of y alone; everything else is exp2(y log2 x)
    'POW': [((NAN, 2), NAN), ((2, NAN), NAN), ((NAN, 0), NAN), ((1, NAN), NAN), ((-1.5, 2), NAN), ((-INF, 2), NAN), ((-1.5, INF), NAN),
            ((0, 4.14), 0), ((-0.0, 4.14), 0), ((0, INF), 0), ((0, 0), INF), ((0, -0.0), INF), ((0, -4.14), INF), ((0, -INF), INF),
            ((INF, 4.14), INF), ((INF, INF), INF), ((INF, 0), 0), ((INF, -4.14), 0), ((INF, -INF), 0),
            ((1, INF), NAN), ((1, -INF), NAN), ((1, 4.14), 1), ((1, -4.14), 1), ((2, 0), 1), ((0.3, -0.0), 1), ((3e38, 0), 1), ((1e-45, 0), 1),
            ((2, INF), INF), ((2, -INF), 0), ((0.5, INF), 0), ((0.5, -INF), INF), ((2, 3), 8), ((2, -2), 0.25), ((2, 128), INF), ((2, -150), 0),
            ((2, -149), 2.0 ** -149), ((2, 127), 2.0 ** 127), ((1e-45, 1), 2.0 ** -149), ((3e38, 2), INF), ((1e-30, 2), 0)],
    'POW_POSEXP': [((NAN,), NAN), ((-1.5,), NAN), ((-INF,), NAN), ((0.0,), 0), ((-0.0,), 0), ((INF,), INF), ((1.0,), 1)],
    'ACOS': [((NAN,), NAN), ((1.0000001,), NAN), ((-1.0000001,), NAN), ((2.0,), NAN), ((INF,), NAN), ((-INF,), NAN), ((1.0,), 0), ((-1.0,), PI32),
             ((0.0,), PIO2_32), ((-0.0,), PIO2_32), ((1e-45,), PIO2_32), ((0.5,), float(F32(np.pi / 3))), ((-0.5,), float(F32(2 * np.pi / 3)))],
    'ATANH': [((1.0,), INF), ((-1.0,), -INF), ((1.0000001,), NAN), ((-2.0,), NAN), ((INF,), NAN), ((-INF,), NAN), ((NAN,), NAN), ((0.0,), 0), ((-0.0,), 0),
              ((1e-45,), 0), ((-1e-20,), 0)],
    'EXP': [((NAN,), NAN), ((INF,), INF), ((-INF,), 0), ((0.0,), 1), ((-0.0,), 1), ((89.0,), INF), ((1e30,), INF), ((-110.0,), 0), ((-1e30,), 0), ((1e-45,), 1)],
    'NORM3': [((INF, 1, 2), INF), ((1, -INF, 2), INF), ((NAN, 1, 2), NAN), ((1, 2, NAN), NAN), ((INF, NAN, 0), NAN), ((3, 4, 0), 5), ((0, 0, 0), 0),
              ((-0.0, 0, -0.0), 0), ((3e38, 0, 0), 3e38), ((3e38, 3e38, 0), INF), ((2e38, 2e38, 1e38), 3e38), ((1e-45, 0, 0), 1e-45), ((0, -3e-39, 4e-39), 5e-39)],
    'DOT3': [((NAN, 0, 0, 1, 1, 1), NAN), ((1, 1, 1, 0, NAN, 0), NAN), ((INF, 0, 0, 1, 1, 1), INF), ((INF, 0, 0, 0, 1, 1), NAN), ((INF, INF, 0, 1, -1, 1), NAN),
             ((3e38, 3e38, 1, 2, -2, 1), NAN), ((3e38, 0, 1, 2, 5, 1), INF), ((1, 2, 3, 4, 5, 6), 32), ((0, 0, 0, 0, 0, 0), 0), ((1e-30, 0, 0, 1e-30, 0, 0), 0),
             ((3e38, 3e38, 3e38, 0.5, 0.5, 0.5), INF), ((1e19, 1, 1, 1e19, -1, 0), 1e38)],
    'WRAP_PI': [((NAN,), NAN), ((INF,), NAN), ((-INF,), NAN), ((0.0,), 0), ((-0.0,), 0), ((float(ms.TWO_PI_F),), 0), ((-float(ms.TWO_PI_F),), 0), ((PI32,), PI32),
                ((-PI32,), PI32), ((float(np.nextafter(ms.PI_F, F32(4))),), float(F32(np.nextafter(ms.PI_F, F32(4)) - ms.TWO_PI_F))), ((-1e-42,), 0), ((1e-42,), 1e-42)],
}


@pytest.mark.parametrize('fn', sorted(SPECIAL))
def test_special_values_follow_the_ladders_of_the_code(fn):
    rows = SPECIAL[fn]
    x = np.array([r[0] for r in rows], F32)
    want = np.array([np.atleast_1d(r[1]) for r in rows], np.float64).astype(F32)
    got = fo.math_array(fn, x, ms.ATM_EXP)
    bad = [(rows[i][0], got[i].tolist(), want[i].tolist()) for i in np.nonzero(~_same(got, want).all(1))[0]]
    assert not bad, bad
    # NaN in -> NaN out for every function, in every position, over the whole grid
    for xb, p in ms.batches(fn)[:2]:
        nan = np.isnan(xb).any(1)
        assert nan.any() and np.isnan(fo.math_array(fn, xb[nan], p)).all(), fn


# ---- the controller's fp32 nonlinearities ------------------------------------------------------------------------------------------
def test_act_functions_against_fp64_libm():
    """act_exp, act_sigmoid, act_tanh (csrc/np_actor.h == oracle/f16_actor.inc) over the grid and the edge list against numpy fp64: the measured
    maxima (math_spec.ACT_*: act_exp relative on [-87, 88], the others absolute) are asserted with a factor 2 for another host's libm; range,
    saturation, NaN and the normal-number property of act_exp are asserted outright."""
    x = ms.batches('ACT_EXP')[0][0][:, 0]
    nn = ~np.isnan(x)
    with np.errstate(all='ignore'):
        xd = x.astype(np.float64)
    e, s, t = (fo.math_array(fn, x)[:, 0] for fn in ('ACT_EXP', 'ACT_SIGMOID', 'ACT_TANH'))
    assert np.isnan(e[~nn]).all() and np.isnan(s[~nn]).all() and np.isnan(t[~nn]).all()
    # act_exp: clamped argument, a normal number for every non-NaN input
    with np.errstate(all='ignore'):
        xc = np.clip(x, F32(-87), F32(88))
        assert _same(e, fo.math_array('ACT_EXP', xc)[:, 0]).all()
        assert (np.abs(e[nn]) >= 2.0 ** -126).all() and np.isfinite(e[nn]).all() and (e[nn] > 0).all()
        inr = nn & (x >= -87) & (x <= 88)
        rel = np.abs(e[inr].astype(np.float64) - np.exp(xd[inr])) / np.exp(xd[inr])
        sig = np.abs(s[nn].astype(np.float64) - 1.0 / (1.0 + np.exp(-xd[nn])))
        tnh = np.abs(t[nn].astype(np.float64) - np.tanh(xd[nn]))
    _report('act_exp', inputs=int(inr.sum()), max_rel_error=float(rel.max()), at=float(x[inr][np.argmax(rel)]))
    _report('act_sigmoid', inputs=int(nn.sum()), max_abs_error=float(sig.max()), at=float(x[nn][np.argmax(sig)]))
    _report('act_tanh', inputs=int(nn.sum()), max_abs_error=float(tnh.max()), at=float(x[nn][np.argmax(tnh)]))
    print('act_exp max rel', rel.max(), 'act_sigmoid max abs', sig.max(), 'act_tanh max abs', tnh.max())
    assert rel.max() <= 2 * ms.ACT_EXP_MAX_REL
    assert sig.max() <= 2 * ms.ACT_SIGMOID_MAX_ABS
    assert tnh.max() <= 2 * ms.ACT_TANH_MAX_ABS
    # what follows from the formulas alone
    assert (s[nn] >= 0).all() and (s[nn] <= 1).all() and (t[nn] >= -1).all() and (t[nn] <= 1).all()
    v = lambda fn, a: float(fo.math_array(fn, np.array([a], F32))[0, 0])        # noqa: E731
    assert v('ACT_TANH', np.inf) == 1 and v('ACT_TANH', -np.inf) == -1 and v('ACT_SIGMOID', np.inf) == 1
    assert v('ACT_TANH', 44.0) == 1 and v('ACT_TANH', -44.0) == -1 and v('ACT_TANH', 0.0) == 0 and v('ACT_SIGMOID', 0.0) == 0.5 and v('ACT_EXP', 0.0) == 1
    lo = v('ACT_SIGMOID', -np.inf)                                              # 1 / (1 + e^88): an fp32 denormal quotient, not flushed
    assert 0 < lo < 2.0 ** -126 and lo == float(F32(1) / (F32(1) + F32(v('ACT_EXP', 88.0))))
    # monotone where the argument is far from a rounding plateau: saturation is reached and kept
    assert (t[nn & (x > 10)] == 1).all() and (t[nn & (x < -10)] == -1).all() and (s[nn & (x > 20)] == 1).all()
