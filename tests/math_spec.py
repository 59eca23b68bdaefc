"""Shared pieces of the elementary-function tests (tests/test_math_spec_cpu.py, tests/test_gpu_math_twins.py): the input sets — the
all-binade grid and one edge list per function — and the host-side classification that says which branch of the written sequence
(csrc/np_math.h, csrc/np_actor.h == oracle/f16_oracle.c, f16_combat.inc, f16_actor.inc) a row reaches.

TEST INFRASTRUCTURE ONLY.  Nothing here evaluates the functions under test: the classes are read off the input values with numpy
fp64, so that a set which silently loses an edge fails the test that uses it.
"""
import functools

import numpy as np

from oracle.f16_oracle import MATH_COLS, MATH_FN  # noqa: F401  (re-exported: ids and column counts of f16o_math_array / np_selfcheck_math)

F32 = np.float32
INVPIO2 = 6.36619772367581382433e-01
TWO_PI_D = 6.283185307179586476925
TWO_PI_F = F32(6.28318530717958647692)
PI_F = F32(3.14159265358979323846)
SQRT2 = 1.4142135623730951
ACT_LOG2E = F32(1.44269504)
MAX_ROWS = 1 << 23                      # rows per launch of the GPU tests
ATM_EXP = float(F32(4.14))              # np_f16_airframe.atm_exp as the device holds it: (double)(float)4.14
POSEXP_PARAMS = (ATM_EXP, 0.5, 1.0, 4.14, 50.0)
POW_Y = np.array([4.14, 0.0, -0.0, -4.14, np.inf, -np.inf, np.nan], F32)

# act_exp / act_sigmoid / act_tanh are fp32 approximations without an analytic bound in the project.  These are the errors MEASURED by
# tests/test_math_spec_cpu.py::test_act_functions_against_fp64_libm against numpy's fp64 exp / tanh over the whole grid and the edge lists
# (act_exp: relative, arguments in [-87, 88]; the other two: absolute); the test asserts at twice these values — the margin covers another
# host's libm, the reference is fp64 libm and never the code under test.
ACT_EXP_MAX_REL = 2.2484e-7          # at x = -37.083366
ACT_SIGMOID_MAX_ABS = 9.8496e-8      # at x = 0.3463594
ACT_TANH_MAX_ABS = 1.9699e-7         # at x = -0.1731797


def _ro(a):
    a.setflags(write=False)
    return a


def nbrs(v, d=4):
    """Every value with its d float32 neighbours on either side."""
    v = np.asarray(v, F32).reshape(-1)
    out, up, dn = [v], v, v
    for _ in range(d):
        up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
        out += [up, dn]
    return np.concatenate(out)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(np.float64)


def _pm(v):
    v = np.asarray(v, F32).reshape(-1)
    return np.concatenate([v, -v])


DENORMALS = _pm(np.array([1, 2, 0x400000, 0x7FFFFF, 0x800000], np.uint32).view(F32))      # + the smallest normal number
SPECIALS = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F32), DENORMALS])


@functools.lru_cache(maxsize=None)
def grid():
    """Both signs x 256 exponent fields x (first 8, last 8 and 2^13 evenly strided significands): 4 202 496 floats with the zeros, the
    denormals, the infinities and NaNs; shuffled with a fixed seed so that one wave holds mixed branches."""
    sig = np.concatenate([np.arange(8), np.arange((1 << 23) - 8, 1 << 23), np.arange(1 << 13) * 1024 + 517]).astype(np.uint32)
    e = np.arange(256, dtype=np.uint32)
    bits = (e[:, None] << 23) | sig[None, :]
    bits = np.concatenate([bits.reshape(-1), bits.reshape(-1) | np.uint32(0x80000000)])
    assert bits.size == np.unique(bits).size == 2 * 256 * (16 + (1 << 13))
    return _ro(bits[np.random.RandomState(20261021).permutation(bits.size)].view(F32))


# ---- edge lists ------------------------------------------------------------------------------------------------------------------
def _sincos_edges():
    rng = np.random.RandomState(11)
    kmax = int(2.0 ** 30 * 2 / np.pi)
    k = np.concatenate([np.arange(65), rng.randint(65, kmax, 2000)]).astype(np.float64)
    kt = np.concatenate([np.arange(65), rng.randint(65, kmax, 300)]).astype(np.float64) + 0.5            # rint ties of x * 2/pi
    big = np.exp(np.linspace(np.log(2.0 ** 30), np.log(3e38), 1000))
    return _pm(np.concatenate([nbrs(k * (np.pi / 2)), nbrs(kt * (np.pi / 2)), nbrs(2.0 ** 30), nbrs(big), SPECIALS]))


_POW_BASES = None


def _pow_bases():
    global _POW_BASES
    if _POW_BASES is None:
        seam = nbrs(np.array([SQRT2 * 2.0 ** e for e in (-140, -127, -126, -20, -1, 0, 1, 20, 127)]))
        _POW_BASES = np.concatenate([seam, nbrs(1.0), SPECIALS, np.array([-1.5, 0.05, 0.5, 1.3, 2.0, 3e38], F32),
                                     np.linspace(0.05, 1.3, 400).astype(F32)])
    return _POW_BASES


_POW_TARGETS = (126, 127, 128, 149, 150, 1022, 1024, 1074, 1075, 2000)


def _pow_edges():
    b = _pow_bases()
    rows = [np.stack([np.repeat(b, POW_Y.size), np.tile(POW_Y, b.size)], 1)]
    for base in np.array([2.0, 0.5, 1.5, 1e-40, 3e38, np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))], F32):
        lg = np.log2(np.float64(base))
        y = nbrs(np.array([s * P / lg for P in _POW_TARGETS for s in (1, -1)]))
        rows.append(np.stack([np.full(y.size, base, F32), y], 1))
    return np.concatenate(rows).astype(F32)


def _exp_edges():
    c = np.array([87.3, -87.3, -103.3, 88.73, -88.73, 1386.2943, -1386.2943, 103.97, -103.97, 709.78, -745.13], np.float64)
    return np.concatenate([nbrs(c), SPECIALS, np.linspace(-104.5, -86.5, 400).astype(F32), np.linspace(-16, 0, 200).astype(F32),
                           np.linspace(-1400, 1400, 561).astype(F32)])


def _acos_edges():
    return np.concatenate([nbrs(_pm([0.5, 1.0])), _pm(np.linspace(1.0, 2.0, 21)[1:]), SPECIALS, np.linspace(-1, 1, 2001).astype(F32)])


def atanh_reachable(x):
    """The arguments the reward can hand to np_atanh (csrc/np_f16_combat.h::orientation_reward_v2): 1.0f - m with m = max(1.9 TA / pi, 1e-4),
    TA = acos(.) in [0, pi].  m is a float in [1e-4, 1.9 (+ an ulp)], so the argument lies in [-0.9000001, 1 - 1e-4] and is a multiple of
    2^-24 (1 - m is exact for m >= 0.5 and a float in [0.5, 1) otherwise)."""
    x = np.asarray(x, F32).astype(np.float64)
    s = x * 2.0 ** 24
    return (x >= -0.9000001) & (x <= 1.0 - 1e-4 + 1e-9) & (s == np.rint(s))


def _atanh_edges():
    m = np.exp(np.linspace(np.log(1e-4), np.log(1.9), 4000)).astype(F32)
    m = np.concatenate([m, nbrs(np.array([1e-4, 0.5, 1.0, 1.9], F32))])
    m = m[(m >= F32(1e-4)) & (m <= np.nextafter(F32(1.9), F32(2)))]
    reach = F32(1.0) - m
    return np.concatenate([nbrs(_pm([1.0])), _pm([1.5, 2.0, 1e10]), _pm(2.0 ** -np.arange(1, 150.0)), reach,
                           (np.arange(-64, 65) * 2.0 ** -24).astype(F32), SPECIALS])


_BIG = np.array([1e19, 1.8446744e19, 1.9e19, 3e19, 1e25, 1e30, 1e38, 3e38, 3.4028235e38], F32)


def _with_nonfinite(rows, cols):
    """`rows` plus, per position, a copy of the first rows with inf, -inf and NaN there, and inf next to NaN."""
    out = [rows]
    for p in range(cols):
        for v in (np.inf, -np.inf, np.nan):
            r = rows[:4].copy()
            r[:, p] = v
            out.append(r)
        r = rows[:2].copy()
        r[:, p], r[:, (p + 1) % cols] = np.inf, np.nan
        out.append(r)
    return np.concatenate(out).astype(F32)


def _norm3_edges():
    rng = np.random.RandomState(12)
    a, b, c = np.meshgrid(_BIG, _BIG, _BIG, indexing='ij')
    big = np.stack([a.reshape(-1), b.reshape(-1), c.reshape(-1)], 1)
    big = np.concatenate([big, big * np.array([1, -1, 1], F32), big * np.array([-1, -1, -1], F32)])
    den = DENORMALS[rng.randint(0, DENORMALS.size, (200, 3))]
    plain = np.concatenate([np.array([[1, 2, 3], [3, 4, 0], [0, 0, 0], [-0.0, 0, -0.0], [3e38, 1e-45, 1], [1e-45, 0, 0], [2.4e38, 2.4e38, 0]], F32),
                            rng.normal(0, 1000, (500, 3)).astype(F32)])
    return _with_nonfinite(np.concatenate([plain, big, den]), 3)


def _dot3_edges():
    rng = np.random.RandomState(13)
    t, u, s, v = (rng.normal(0, 1000, 600).astype(F32) for _ in range(4))
    cancel = np.stack([t, t, s, u, -u, v], 1)                                   # a0 b0 == -(a1 b1): the sum is the third product
    cancel2 = np.stack([t, u, s * F32(1e-6), u, -t, v * F32(1e-6)], 1)
    i = rng.randint(0, _BIG.size, (400, 6))
    big = _BIG[i] * rng.choice(np.array([1, -1], F32), (400, 6))
    mixed = big.copy()
    mixed[:, 3:] = rng.uniform(-2, 2, (400, 3)).astype(F32)
    den = DENORMALS[rng.randint(0, DENORMALS.size, (200, 6))]
    tiny = rng.normal(0, 1, (200, 6)).astype(F32) * F32(1e-20)
    plain = np.array([[1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0], [3e38, 3e38, 1, 2, -2, 1], [1e19, 1, 1, 1e19, 1, 1]], F32)
    return _with_nonfinite(np.concatenate([plain, cancel, cancel2, big, mixed, den, tiny]), 6)


def _wrap_edges():
    rng = np.random.RandomState(2)
    c = np.float64(TWO_PI_F)
    k = rng.randint(-160000, 160000, 2000).astype(np.float64)
    special = np.array([0.0, -0.0, c, -c, 2 * c, np.pi, -np.pi, np.nextafter(F32(np.pi), F32(4)), 1e-42, -1e-42, 1048575.94,
                        1048576.0, 1048576.1, -1048576.0, 3e7, -3e7, 1e30, -1e30, np.inf, -np.inf, np.nan, 1.17549435e-38], F32)
    kk = np.concatenate([np.arange(-40, 41.0), k])
    return np.concatenate([special, nbrs(kk * c), nbrs(kk * c + np.pi), nbrs(_pm(np.exp(np.linspace(np.log(20), np.log(3e38), 500)))), SPECIALS,
                           rng.uniform(-20, 20, 1000).astype(F32)])


def _act_edges():
    k = np.arange(-127, 128.0) + 0.5
    ties = nbrs(k / np.float64(ACT_LOG2E))                                      # arguments of act_exp whose x * 1.44269504f is k + 1/2
    clamps = nbrs(np.array([-87.0, 88.0, -43.5, 44.0, 87.3365, 43.66825, 88.7228, 44.3614]))
    a = np.concatenate([ties, clamps])
    return np.concatenate([_pm(a), _pm(a * F32(0.5)), SPECIALS, np.linspace(-12, 12, 2401).astype(F32)])


_EDGES = {'SINCOS': _sincos_edges, 'SINCOSTAN': _sincos_edges, 'POW': _pow_edges, 'POW_POSEXP': _pow_bases, 'ACOS': _acos_edges,
          'ATANH': _atanh_edges, 'EXP': _exp_edges, 'NORM3': _norm3_edges, 'DOT3': _dot3_edges, 'WRAP_PI': _wrap_edges,
          'ACT_EXP': _act_edges, 'ACT_SIGMOID': _act_edges, 'ACT_TANH': _act_edges}


@functools.lru_cache(maxsize=None)
def edges(fn):
    """The edge list of a function as rows [m, in_cols] float32."""
    with np.errstate(all='ignore'):
        e = np.asarray(_EDGES[fn](), F32)
    return _ro(np.ascontiguousarray(e.reshape(-1, MATH_COLS[fn][0])))


def _grid_columns(fn):
    """The grid as rows of the 3- and 6-column functions: once with every component from another (shuffled) binade, once with components
    of comparable magnitude so that the sums are not decided by one term."""
    g = grid()
    if fn == 'NORM3':
        yield np.stack([g, np.roll(g, 1), np.roll(g, 2)], 1)
        yield np.stack([g, g * F32(0.75), g * F32(-1.25)], 1)
    else:
        yield np.stack([np.roll(g, j) for j in range(6)], 1)
        u = np.random.RandomState(14).uniform(-2, 2, (g.size, 3)).astype(F32)
        yield np.concatenate([np.stack([g, g * F32(0.75), g * F32(-1.25)], 1), u], 1)


def batches(fn):
    """The inputs of one function as a list of (rows [n, in_cols] float32, param), n <= MAX_ROWS each: the whole grid (crossed with the short
    exponent list for the two-argument functions) and the function's edge list, which travels with the first batch."""
    with np.errstate(all='ignore'):
        out = _batches(fn)
    out = [(np.ascontiguousarray(x, F32), p) for x, p in out]
    assert all(x.shape[0] <= MAX_ROWS and x.shape[1] == MATH_COLS[fn][0] for x, _ in out)
    return out


def _batches(fn):
    g, e = grid(), edges(fn)
    if fn == 'POW':
        out = [(np.stack([g, np.full(g.size, y, F32)], 1), 0.0) for y in POW_Y]
        out[0] = (np.concatenate([out[0][0], e]), 0.0)
    elif fn == 'POW_POSEXP':
        out = [(np.concatenate([g, e.reshape(-1)])[:, None], p) for p in POSEXP_PARAMS]
    elif fn in ('NORM3', 'DOT3'):
        out = [(x, 0.0) for x in _grid_columns(fn)]
        out[0] = (np.concatenate([out[0][0], e]), 0.0)
    else:
        out = [(np.concatenate([g, e.reshape(-1)])[:, None], 0.0)]
    return out


# ---- which branch a row reaches, read off the input ------------------------------------------------------------------------------
def _common(x):
    a = np.abs(x)
    return {'nan_in': np.isnan(x), 'inf_in': np.isinf(x), 'zero_in': x == 0, 'denormal_in': (a > 0) & (a < 2.0 ** -126)}


def _sincos_classes(xf):
    x = xf.astype(np.float64)
    fin = np.isfinite(x)
    big = fin & ~(np.abs(x) < 2.0 ** 30)
    with np.errstate(invalid='ignore'):
        xr = np.where(big, np.fmod(x, TWO_PI_D), x)
        t = xr * INVPIO2
        k = np.rint(t)
        r = np.abs(xr - k * (np.pi / 2))
        frac = np.abs(t - k)
    u = ulp32(np.where(fin, xf, 0))
    q = np.where(fin, k, 0).astype(np.int64) & 3
    c = _common(x)
    c.update({'fmod_path': big, 'just_below_2p30': fin & (np.abs(x) < 2.0 ** 30) & (np.abs(x) >= 2.0 ** 30 - 256),
              'at_or_just_above_2p30': big & (np.abs(x) <= 2.0 ** 30 + 512),
              'multiple_of_pio2_within_4ulp': fin & ~big & (k != 0) & (r <= 4.5 * u),
              'rint_tie_within_4ulp': fin & ~big & (0.5 - frac <= 4.5 * u * INVPIO2)})
    for n in range(4):
        c[f'quadrant_{n}'] = fin & ~big & (q == n)
        c[f'fmod_quadrant_{n}'] = big & (q == n)
    return c


def _log_exp_classes(x, P, c):
    """Classes of exp2_d(P) and, where x is given, of log2_d(x) for finite positive x."""
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(P) if x is None else (np.isfinite(x) & (x > 0) & ~np.isnan(P))
        if x is not None:
            m, _ = np.frexp(np.where(ok, x, 1.0))
            m = m * 2.0                                                       # [1, 2)
            c.update({'log_mant_gt_sqrt2': ok & (m > SQRT2), 'log_mant_le_sqrt2': ok & (m <= SQRT2),
                      'log_mant_seam_within_4ulp': ok & (np.abs(m - SQRT2) <= 4.5 * 2.0 ** -23), 'x_is_one': ok & (x == 1.0)})
        c.update({'P_above_clamp_2000': ok & (P > 2000), 'P_below_clamp_m2000': ok & (P < -2000),
                  'result_fp32_denormal': ok & (P < -126) & (P >= -149), 'result_fp64_denormal': ok & (P < -1022) & (P >= -1074),
                  'result_underflows_to_zero': ok & (P < -1075) & (P >= -2000), 'result_overflows_fp32': ok & (P >= 128) & (P < 1024),
                  'result_overflows_fp64': ok & (P >= 1024) & (P <= 2000), 'result_normal': ok & (P > -126) & (P < 127)})
    return c


def _pow_classes(xf, y):
    x = xf.astype(np.float64)
    y = np.asarray(y, np.float64) + np.zeros_like(x)
    nan = np.isnan(x) | np.isnan(y)
    c = {'nan_in': nan, 'x_negative': ~nan & (x < 0), 'x_zero_y_positive': ~nan & (x == 0) & (y > 0),
         'x_zero_y_not_positive': ~nan & (x == 0) & ~(y > 0), 'x_inf_y_positive': ~nan & (x == np.inf) & (y > 0),
         'x_inf_y_not_positive': ~nan & (x == np.inf) & ~(y > 0), 'x_denormal': ~nan & (x > 0) & (x < 2.0 ** -126),
         'y_infinite': ~nan & np.isinf(y) & (x > 0) & np.isfinite(x), 'y_zero': ~nan & (y == 0) & (x > 0) & np.isfinite(x)}
    with np.errstate(invalid='ignore', divide='ignore'):
        P = y * np.log2(np.where(x > 0, x, np.nan))
    c['inf_times_zero'] = ~nan & np.isinf(y) & (x == 1.0)
    return _log_exp_classes(np.where(np.isnan(P) & ~c['inf_times_zero'], np.nan, x), P, c)


def _posexp_classes(xf, y):
    c = _pow_classes(xf, y)
    for k in ('y_infinite', 'y_zero', 'inf_times_zero', 'x_zero_y_not_positive', 'x_inf_y_not_positive'):
        del c[k]                                                               # the exponent is positive and finite by contract
    return c


def _exp_classes(xf):
    x = xf.astype(np.float64)
    return _log_exp_classes(None, x * 1.44269504088896338700, _common(x))


def _acos_classes(xf):
    x = xf.astype(np.float64)
    a = np.abs(x)
    c = _common(x)
    c.update({'small_branch': a < 0.5, 'large_branch_positive': (a >= 0.5) & (x > 0) & (a <= 1), 'large_branch_negative': (a >= 0.5) & (x < 0) & (a <= 1),
              'seam_half_within_4ulp': np.abs(a - 0.5) <= 4.5 * 2.0 ** -25, 'plus_one': x == 1, 'minus_one': x == -1,
              'one_ulp_inside_one': a == np.float64(np.nextafter(F32(1), F32(0))), 'abs_in_1_2': (a > 1) & (a <= 2)})
    return c


def _atanh_classes(xf):
    x = xf.astype(np.float64)
    a = np.abs(x)
    c = _common(x)
    c.update({'plus_one': x == 1, 'minus_one': x == -1, 'abs_above_one': (a > 1) & np.isfinite(a),
              'one_ulp_inside_one': a == np.float64(np.nextafter(F32(1), F32(0))), 'below_half_ulp_of_one': (a > 0) & (a < 2.0 ** -54),
              'reachable': atanh_reachable(xf), 'reachable_near_zero': atanh_reachable(xf) & (a < 2.0 ** -12) & (a > 0),
              'quotient_mant_gt_sqrt2': (a < 1) & (np.frexp((1 + x) / np.where(a < 1, 1 - x, 1))[0] * 2 > SQRT2)})
    return c


FLT_MAX = float(np.finfo(F32).max)


def _norm3_classes(v):
    d = v.astype(np.float64)
    a = np.abs(d)
    fin = np.isfinite(d).all(1)
    with np.errstate(over='ignore', invalid='ignore'):
        n = np.sqrt((d * d).sum(1))
    return {'nan_in': np.isnan(d).any(1), 'inf_in': np.isinf(d).any(1), 'inf_and_nan_in': np.isinf(d).any(1) & np.isnan(d).any(1), 'all_zero': (d == 0).all(1),
            'denormal_component': ((a > 0) & (a < 2.0 ** -126)).any(1), 'all_denormal': ((a > 0) & (a < 2.0 ** -126)).all(1),
            'square_overflows_fp32': fin & (a > 1.8446744e19).any(1), 'every_square_overflows_fp32': fin & (a > 1.8446744e19).all(1),
            'norm_overflows_fp32': fin & (n > FLT_MAX * (1 + 2.0 ** -25)), 'norm_finite_though_squares_overflow': fin & (a > 1.8446744e19).any(1) & (n < FLT_MAX),
            'mixed_signs': fin & (d < 0).any(1) & (d > 0).any(1)}


def _dot3_classes(v):
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        p = (v[:, :3] * v[:, 3:]).astype(F32)                                  # the spec rounds each product to fp32 first
        pd = p.astype(np.float64)
        s = (pd[:, 0] + pd[:, 1]) + pd[:, 2]
        exact = v[:, :3].astype(np.float64) * v[:, 3:].astype(np.float64)
    fin = np.isfinite(v).all(1)
    ap = np.abs(pd)
    mx = ap.max(1)
    return {'nan_in': np.isnan(v).any(1), 'inf_in': np.isinf(v).any(1), 'product_overflows_fp32': fin & np.isinf(p).any(1),
            'inf_minus_inf': fin & (p == np.inf).any(1) & (p == -np.inf).any(1),
            'product_denormal_or_flushed': fin & ((np.abs(exact) > 0) & (np.abs(exact) < 2.0 ** -126)).any(1),
            'cancellation': fin & np.isfinite(s) & (mx > 0) & (np.abs(s) <= mx * 2.0 ** -10),
            'exact_cancellation_of_two': fin & np.isfinite(pd).all(1) & (pd[:, 0] == -pd[:, 1]) & (pd[:, 0] != 0),
            'sum_overflows_fp32': fin & np.isfinite(pd).all(1) & (np.abs(s) > FLT_MAX * (1 + 2.0 ** -25)), 'all_zero': (v == 0).all(1)}


def _wrap_classes(xf):
    with np.errstate(invalid='ignore'):
        r = np.fmod(xf, TWO_PI_F)                                              # exact in fp32
    fin = np.isfinite(xf)
    c = _common(xf.astype(np.float64))
    r1 = np.where(fin & (r < 0), r + TWO_PI_F, r)
    c.update({'negative_zero_in': (xf == 0) & np.signbit(xf), 'exact_multiple_of_2pi_f': fin & (xf != 0) & (r == 0),
              'negative_remainder': fin & (r < 0), 'remainder_above_pi': fin & (r1 > PI_F), 'remainder_is_pi': fin & (r1 == PI_F),
              'negative_remainder_rounds_to_2pi_f': fin & (r < 0) & (r1 == TWO_PI_F), 'huge': fin & (np.abs(xf) >= F32(2.0 ** 24) * TWO_PI_F)})
    return c


def _act_exp_classes(xf, name=''):
    """Classes of act_exp(x) on its argument (the callers hand over -x and 2x)."""
    with np.errstate(invalid='ignore', over='ignore'):
        xc = np.minimum(np.maximum(xf, F32(-87)), F32(88))
        t = (xc * ACT_LOG2E).astype(F32)
        k = np.rint(t)
        tie = (np.abs(t - np.floor(t)) == F32(0.5)) & np.isfinite(t)
    nn = ~np.isnan(xf)
    return {name + 'below_clamp_m87': nn & (xf < -87), name + 'above_clamp_88': nn & (xf > 88), name + 'at_clamp_m87': xf == -87, name + 'at_clamp_88': xf == 88,
            name + 'rintf_tie': nn & tie, name + 'k_is_m126': nn & (k == -126), name + 'k_is_127': nn & (k == 127), name + 'k_is_zero': nn & (k == 0)}


def _act_classes(fn, xf):
    c = _common(xf.astype(np.float64))
    if fn == 'ACT_EXP':
        c.update(_act_exp_classes(xf))
    elif fn == 'ACT_SIGMOID':
        c.update(_act_exp_classes(-xf, 'exp_arg_'))
        c.update({'minus_inf_in': xf == -np.inf, 'denormal_quotient': xf < F32(-87.34)})
    else:
        c.update(_act_exp_classes(F32(2) * xf, 'exp_arg_'))
        c.update({'saturates_to_plus_one': xf > 10, 'saturates_to_minus_one': xf < -10})
    return c


def classes(fn, x, param=0.0):
    """{edge class: mask[n]} of the rows x [n, in_cols] of function `fn`: which branch of the written sequence the row reaches."""
    with np.errstate(all='ignore'):
        return _classes(fn, np.asarray(x, F32), param)


def _classes(fn, x, param):
    if fn in ('SINCOS', 'SINCOSTAN'):
        return _sincos_classes(x[:, 0])
    if fn == 'POW':
        return _pow_classes(x[:, 0], x[:, 1])
    if fn == 'POW_POSEXP':
        return _posexp_classes(x[:, 0], param)
    if fn == 'EXP':
        return _exp_classes(x[:, 0])
    if fn == 'ACOS':
        return _acos_classes(x[:, 0])
    if fn == 'ATANH':
        return _atanh_classes(x[:, 0])
    if fn == 'NORM3':
        return _norm3_classes(x)
    if fn == 'DOT3':
        return _dot3_classes(x)
    if fn == 'WRAP_PI':
        return _wrap_classes(x[:, 0])
    return _act_classes(fn, x[:, 0])


def class_counts(fn):
    """Rows per edge class over all batches of a function."""
    total = {}
    for x, p in batches(fn):
        for k, m in classes(fn, x, p).items():
            total[k] = total.get(k, 0) + int(np.count_nonzero(m))
    return total
