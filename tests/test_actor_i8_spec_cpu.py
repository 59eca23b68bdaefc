"""What the controller's block-fixed-point numerics (oracle/f16_actor_i8.inc, restated by csrc/np_actor_i8.h) is worth, piece by piece
on the CPU: the quantiser against exact integers, the header's range claims as assertions, the quantised Linear against the exact dot
product with a derived bound, LayerNorm against fp64, the library's packer against the restatement on networks built on the packer's
edges.  Inputs and classification: tests/actor_i8_spec.py.  Figures go to actor_i8_spec_cpu.json and DESIGN section 9."""
import math

import numpy as np
import pytest

import actor_i8_spec as S
from oracle.f16_oracle import ActorOracle, i8_quantise

RANDOM_ROWS = 200_000
REPORT = {}


def _report(name, **kw):
    from test_gpu_edge_cases import _write_report
    REPORT[name] = kw
    _write_report('actor_i8_spec_cpu.json', REPORT)


def _shipped(golden_dir):
    from neuralplane_amd.actor import pack_ppo_actor
    d = np.load(f'{golden_dir}/actor_kat.npz')
    return pack_ppo_actor({k[4:]: d[k] for k in d.files if k.startswith('sd::')})


def _nets(golden_dir):
    from neuralplane_amd.actor import pack_ppo_actor
    nets = {'shipped': _shipped(golden_dir)}
    nets.update({k: pack_ppo_actor(sd) for k, sd in S.synthetic_nets().items()})
    return nets


def _edge_obs(golden_dir, w):
    """The observation rows found under the shipped LayerNorm 0 and those found under network w's own."""
    return np.concatenate([S.edge_obs_rows(_shipped(golden_dir)), S.edge_obs_rows(w)])


NET_NAMES = ['shipped', 'weight_edges', 'flat_norms', 'steep_norms']


def test_every_class_is_constructed_and_the_emulation_is_the_restatement(golden_dir):
    """The edge rows reach every class (recurrent state: built; observations: found under the shipped LayerNorm 0; weights: the
    weight_edges network), and the numpy emulation of LayerNorm 0 the scan relies on equals f16o_actor_i8_layernorm bit for bit."""
    w = _shipped(golden_dir)
    h, m = S.edge_h_rows()
    got = set().union(*S.h_classes_of(h, m))
    assert not [c for c in S.H_CLASSES if c not in got]
    eo = S.edge_obs_rows(w)
    got = set().union(*S.classify_obs(w, eo))
    assert not [c for c in S.OBS_CLASSES if c not in got]
    rng = np.random.RandomState(1)
    x = np.concatenate([eo, (rng.normal(0, 1, (50_000, 22)) * rng.uniform(0.1, 30, (1, 22))).astype(np.float32)])
    for name, wn in _nets(golden_dir).items():
        y, B, ex = S.ln0_emulate(wn, x)
        y2, ex2 = ActorOracle(wn, 'i8').i8_layernorm(0, x)
        assert S.same_bits(y, y2) and np.array_equal(ex, ex2), name
    sds = S.synthetic_nets()
    wc = set().union(*[S.classify_weights(sds['weight_edges'][S._wkey(L)]) for L in S.LINEARS])
    assert not [c for c in S.W_CLASSES if c not in wc]
    _, B, ex = S.ln0_emulate(_nets(golden_dir)['flat_norms'], x)
    assert (B == 0).all() and (ex == S.CLAMP).all()                       # gamma = beta = 0: the clamp
    assert S.ln0_emulate(_nets(golden_dir)['steep_norms'], x)[2].max() >= 100


def _check_quantiser(x, ex, what):
    """q == round-half-even(x 2^(22 - ex)) in exact arithmetic, the limbs reassemble to q, |q| <= 2^22, the magic sum stays in [2^23, 2^24]."""
    q, limbs, qsum = i8_quantise(x, ex)
    want, _ = S.exact_q(x, np.asarray(ex)[:, None])
    assert np.array_equal(q.astype(np.int64), want), what
    l = limbs.astype(np.int64)
    assert np.array_equal((l[:, 2] * 256 + l[:, 1]) * 256 + l[:, 0], want), what
    assert np.abs(want).max() <= 2 ** 22, (what, int(np.abs(want).max()))
    assert qsum.min() >= 2.0 ** 23 and qsum.max() <= 2.0 ** 24, (what, float(qsum.min()), float(qsum.max()))
    return int(np.abs(want).max())


def test_quantiser_on_the_edge_rows_is_exact_rounding(golden_dir):
    """Every edge row of the recurrent state (quantised with eh = exponent(max |h mask|)) and every edge observation behind LayerNorm 0."""
    h, m = S.edge_h_rows()
    hm = h * m[:, None]
    top = _check_quantiser(hm, S.exponent(np.abs(hm).max(1)), 'recurrent state')
    assert top == 2 ** 22                                                  # reached exactly: the header's "|q| < 2^22" was off by one
    w = _shipped(golden_dir)
    y, ex = ActorOracle(w, 'i8').i8_layernorm(0, S.edge_obs_rows(w))
    _check_quantiser(y, ex, 'observations')
    _report('quantiser_edges', rows_h=int(h.shape[0]), max_abs_q=top)


def _layer_inputs(o, n, seed, edge_obs, edge_h, edge_mask):
    """Inputs (x, ex) of the six quantised layers for n random rows + the edge rows, chained through the restatement's own pieces; the GRU cell
    between GI / GH and LayerNorm 3 is stood in for by the recurrent-state rows themselves (|h| < 1 for the random ones)."""
    rng = np.random.RandomState(seed)
    obs = np.concatenate([edge_obs, (rng.normal(0, 1, (n, 22)) * rng.uniform(0.1, 30, (1, 22))).astype(np.float32)])
    hm = np.concatenate([edge_h * edge_mask[:, None], np.tanh(rng.normal(0, 0.7, (n, 128))).astype(np.float32)])
    out = []
    y, ex = o.i8_layernorm(0, obs); out.append((y, ex))
    a = np.maximum(o.i8_dense(0, y, ex)[0], 0)
    y, ex = o.i8_layernorm(1, a); out.append((y, ex))
    a = np.maximum(o.i8_dense(1, y, ex)[0], 0)
    y, ex = o.i8_layernorm(2, a); out.append((y, ex))
    out.append((hm, S.exponent(np.abs(hm).max(1)).astype(np.int32)))
    with np.errstate(all='ignore'):
        hfin = np.where(np.abs(hm) < 1e30, hm, np.float32(0.5))            # LayerNorm 3 of a row with 3e38 in it overflows its sum: not this test's subject
    y, ex = o.i8_layernorm(3, hfin); out.append((y, ex))
    a = np.maximum(o.i8_dense(4, y, ex)[0], 0)
    y, ex = o.i8_layernorm(4, a); out.append((y, ex))
    return out


@pytest.mark.parametrize('net', NET_NAMES)
def test_range_claims_hold_on_edge_rows_and_200000_random_rows_per_layer(golden_dir, net):
    """The header's claims as assertions, violations allowed: 0 — |q| <= 2^22 for every quantised value, fmaf(x, scale, magic) inside
    [2^23, 2^24] (where the magic-number rounding is exact), every class sum |c_i| < 2^24 (so its conversion to fp32 is exact)."""
    w = _nets(golden_dir)[net]
    o = ActorOracle(w, 'i8')
    eh, em = S.edge_h_rows()
    worst_q, worst_c = 0, np.zeros(4, np.int64)
    for layer, (x, ex) in enumerate(_layer_inputs(o, RANDOM_ROWS, 7, _edge_obs(golden_dir, w), eh, em)):
        worst_q = max(worst_q, _check_quantiser(x, ex, (net, layer)))
        for i0 in range(0, x.shape[0], 50_000):
            _, c = o.i8_dense(layer, x[i0:i0 + 50_000], ex[i0:i0 + 50_000])
            worst_c = np.maximum(worst_c, np.abs(c.astype(np.int64)).max((0, 1)))
    assert worst_c.max() < 2 ** 24, worst_c
    _report(f'ranges/{net}', rows_per_layer=RANDOM_ROWS, max_abs_q=worst_q, max_abs_class_sums=[int(v) for v in worst_c])


def _linear_bound(K, ex, ew, y):
    """|y_j - (sum_k W[j][k] x[k] + b_j)| <= this.  With xq = q 2^(ex - 22), Wq = wq 2^(ew - 29):
       quantisation   |x - xq| <= 2^(ex - 23), |W - Wq| <= 2^(ew - 30), |xq| <= 2^ex, |W| < 2^ew:
                      |sum W x - sum Wq xq| <= K 2^(ex + ew) (2^-23 + 2^-30)
       dropped limbs  per k: |x1.w0 + x0.w1| 2^8 + |x0.w0| <= 2 . 2^14 . 2^8 + 2^14 units of 2^(ex + ew - 51): K 2^(ex + ew) 2^-28 (1 + 2^-9)
       fmaf chain     three roundings of partial sums no larger than the retained sum <= K 2^(ex + ew) (1 + 2^-20): 3 . 2^-24 of it; the
                      two scalings are by powers of two; the last fmaf rounds the result once: 2^-24 |y| (+ 2^-149 when it is denormal)."""
    s = K * np.ldexp(1.0, ex[:, None] + ew[None, :])
    return s * (2.0 ** -23 + 2.0 ** -30 + 2.0 ** -28 * (1 + 2.0 ** -9) + 3 * 2.0 ** -24 * (1 + 2.0 ** -20)) + 2.0 ** -24 * np.abs(y) + 2.0 ** -149


@pytest.mark.parametrize('net', NET_NAMES)
def test_quantised_linear_against_the_exact_dot_product(golden_dir, net):
    """y_j of f16o_actor_i8_dense against sum_k W[j][k] x[k] + b_j (products of fp32 values are exact in fp64, summed with math.fsum), on the
    edge rows and 48 random rows per layer (rows whose exponent is 106 or more are left out and counted: there u * 2^(ex - 17) can overflow): within the bound DERIVED in _linear_bound; and the header's sentence about the dropped limb
    products as the statement it makes — their sum is below 2^-24 of the BOUND on the sum, K 2^(ex + ew) (not of a cancelled sum)."""
    w = _nets(golden_dir)[net]
    o = ActorOracle(w, 'i8')
    eh, em = S.edge_h_rows()
    ratio, rel, drop, beyond = 0.0, 0.0, 0.0, 0
    for layer, (x, ex) in enumerate(_layer_inputs(o, 48, 9, _edge_obs(golden_dir, w), eh, em)):
        n_in, n_out = ActorOracle.LAYER_SHAPES[layer]
        bias, Wt = _linear_terms(w, layer)
        wq, ew = o.quantised_weights(layer)
        assert np.array_equal(ew, S.exponent(np.abs(Wt).max(0).astype(np.float32))), layer      # the layout above is the restatement's
        y, c = o.i8_dense(layer, x, ex)
        q = S.exact_q(x, np.asarray(ex)[:, None])[0]
        full = q @ wq.astype(np.int64).T                                                         # exact: |.| < 2^59
        c = c.astype(np.int64)
        kept = (((c[:, :, 0] * 256 + c[:, :, 1]) * 256 + c[:, :, 2]) * 256 + c[:, :, 3]) * 65536
        drop = max(drop, float(np.abs(full - kept).max() / (n_in * 2.0 ** 51)))
        xd = x.astype(np.float64)
        bound = _linear_bound(n_in, np.asarray(ex, np.int64), ew.astype(np.int64), y)
        assert np.isfinite(y[np.asarray(ex) < 106]).all(), layer          # an infinite output can only come from a row exponent of 106 or more
        for i in range(x.shape[0]):
            if ex[i] >= 106:        # u * 2^(ex - 17) may overflow whatever the weights: the forward pass returns NaN for such rows (ai8_row), counted here
                beyond += 1
                continue
            truth, mag = _exact_linear(Wt, bias, xd[i])
            err = np.abs(y[i].astype(np.float64) - truth)
            assert np.isfinite(err).all() and np.isfinite(bound[i]).all(), (layer, i)
            ratio = max(ratio, float((err / bound[i]).max()))
            if (mag > 0).any():
                rel = max(rel, float(((err - 2.0 ** -24 * np.abs(y[i]))[mag > 0] / mag[mag > 0]).max()))
    print(net, 'error / bound', ratio, 'error / sum |W x|', rel, 'dropped / (K 2^(ex+ew))', drop)
    _report(f'linear/{net}', max_error_over_bound=ratio, max_error_beyond_final_rounding_over_sum_abs_products=rel, max_dropped_over_bound_on_sum=drop, rows_with_exponent_106_or_more_left_out=beyond)
    assert drop < 2.0 ** -24
    assert ratio <= 1.0


@pytest.mark.parametrize('net', NET_NAMES)
def test_layernorm_against_fp64_is_no_worse_than_twice_the_fp32_specs(golden_dir, net):
    """y of the i8 restatement's LayerNorm (lane-block summation order) against LayerNorm in fp64 of the same fp32 inputs; the yardstick is the
    FIRST spec's LayerNorm (f16_actor.inc, 16-wide runs) against the same truth on the same rows: only the order differs, so at most twice —
    asserted for the edge rows (the observation rows of both LayerNorm 0s, the recurrent-state rows below 2^105: larger ones never reach a
    LayerNorm, ai8_row) and for the 20 000 random rows separately, so that a saturated edge row does not hide the others."""
    w = _nets(golden_dir)[net]
    o = ActorOracle(w, 'i8')
    eh, em = S.edge_h_rows()
    ins = _layer_inputs(o, 20_000, 13, _edge_obs(golden_dir, w), eh, em)
    rng = np.random.RandomState(3)
    figures = {}
    for which in range(6):
        n = 22 if which == 0 else 128
        if which == 0:
            x = np.concatenate([_edge_obs(golden_dir, w), (rng.normal(0, 1, (20_000, 22)) * rng.uniform(0.1, 30, (1, 22))).astype(np.float32)])
        elif which == 3:
            hm = eh * em[:, None]
            x = np.concatenate([hm[np.abs(hm).max(1) < 2.0 ** 105], np.tanh(rng.normal(0, 0.7, (20_000, 128))).astype(np.float32)])
        else:
            x = np.maximum(o.i8_dense({1: 0, 2: 1, 4: 4, 5: 5}[which], *ins[{1: 0, 2: 1, 4: 4, 5: 5}[which]])[0], 0)
        g, b = _ln_terms(w, which)
        xd = x.astype(np.float64)
        mean = xd.mean(1, keepdims=True)
        truth = (xd - mean) / np.sqrt(((xd - mean) ** 2).mean(1, keepdims=True) + np.float64(np.float32(1e-5))) * g + b
        d8, d32 = np.abs(o.i8_layernorm(which, x)[0] - truth).max(1), np.abs(o.fp32_layernorm(which, x) - truth).max(1)
        for group, sl in (('edge', slice(0, x.shape[0] - 20_000)), ('random', slice(x.shape[0] - 20_000, None))):
            e8, e32 = float(d8[sl].max()), float(d32[sl].max())
            figures[f'ln{which}/{group}'] = {'i8_order_max_abs_error': e8, 'fp32_spec_max_abs_error': e32}
            print(net, which, group, e8, e32)
            assert e8 <= 2 * e32, (which, group, e8, e32)
    _report(f'layernorm/{net}', **figures)


def _offsets():
    """name -> (offset, size) in the packed buffer, from the packer's own table (neuralplane_amd/actor.py::_LAYOUT)."""
    from neuralplane_amd.actor import _LAYOUT, _SHAPES
    out, p = {}, 0
    for name, key, _ in _LAYOUT:
        n = int(np.prod(_SHAPES[key])) if key in _SHAPES else (22 if name.startswith('ln0') else 384 if name in ('gi_b', 'gh_b') else 4 if name == 'hd_b' else 128)
        out[name] = (p, n)
        p += n
    return out


def _linear_terms(w, layer):
    """(bias [n_out], W^T [n_in, n_out]) float64 of quantised Linear `layer`."""
    n_in, n_out = ActorOracle.LAYER_SHAPES[layer]
    name = ('l1', 'l2', 'gi', 'gh', 'a1', 'a2')[layer]
    off = _offsets()
    (b0, _), (w0, _) = off[name + '_b'], off[name + '_w']
    return w[b0:b0 + n_out].astype(np.float64), w[w0:w0 + n_in * n_out].reshape(n_in, n_out).astype(np.float64)


def _ln_terms(w, which):
    """gamma, beta (float64) of LayerNorm `which`."""
    off = _offsets()
    (g0, n), (b0, _) = off[f'ln{which}_g'], off[f'ln{which}_b']
    return w[g0:g0 + n].astype(np.float64), w[b0:b0 + n].astype(np.float64)


def _exact_linear(Wt, bias, x):
    """sum_k W[j][k] x[k] + b_j for one row, exactly rounded: the products of fp32 values are exact in fp64, math.fsum adds them without error."""
    prod = Wt * x[:, None]
    return np.array([math.fsum(col) + 0.0 for col in np.vstack([prod, bias[None, :]]).T]), np.abs(prod).sum(0)


@pytest.mark.parametrize('net', ['weight_edges', 'flat_norms', 'steep_norms'])
def test_packer_agrees_with_the_restatement_on_the_synthetic_networks(golden_dir, net):
    """np_actor_pack_i8 (host code of the library) against f16o_actor_i8_weights on networks whose rows sit on the packer's edges: limbs, ew,
    the scale table, the LayerNorm bound constants (the shipped weights: tests/test_host_logic_cpu.py)."""
    from neuralplane_amd.actor import NUM_FLOATS, pack_i8
    w = _nets(golden_dir)[net]
    out = pack_i8(w)
    o = ActorOracle(w, 'i8')
    frag = out[NUM_FLOATS + 4368:].view(np.uint8)
    sw_off, base = NUM_FLOATS, 0
    for layer, (n_in, n_out) in enumerate(ActorOracle.LAYER_SHAPES):
        ks_count = 1 if layer == 0 else 4
        wq, ew = o.quantised_weights(layer)
        blocks = n_out // 32
        f = frag[base: base + blocks * ks_count * 4 * 1024].reshape(blocks, ks_count, 4, 64, 16).astype(np.int64)
        f = np.where(f >= 128, f - 256, f)
        val = ((f[:, :, 3] * 256 + f[:, :, 2]) * 256 + f[:, :, 1]) * 256 + f[:, :, 0]
        got = np.zeros((n_out, 32 * ks_count), np.int64)
        for ks in range(ks_count):
            for hh in range(2):
                for e in range(16):
                    got[:, 32 * ks + 8 * (e >> 2) + 4 * hh + (e & 3)] = val[:, ks, 32 * hh: 32 * hh + 32, e].reshape(-1)
        assert np.array_equal(got[:, :n_in], wq) and not got[:, n_in:].any(), layer
        assert np.array_equal(out[sw_off: sw_off + n_out], np.ldexp(np.float32(1), ew - 18).astype(np.float32)), layer
        sw_off += n_out
        base += blocks * ks_count * 4 * 1024
    lnmax = out[NUM_FLOATS + 4356: NUM_FLOATS + 4356 + 12]
    for which in range(6):
        g, b = _ln_terms(w, which)
        assert lnmax[2 * which] == np.float32(np.abs(g).max()) and lnmax[2 * which + 1] == np.float32(np.abs(b).max()), which


@pytest.mark.parametrize('net', NET_NAMES)
def test_non_finite_rows_are_all_nan_whatever_the_sign_and_payload(golden_dir, net):
    """The contract of f16_actor_i8.inc::ai8_row: an infinite or NaN observation, or masked recurrent state (NaN * 0 included), gives NaN in all
    four actions and all 128 states — so rows that differ only in the sign or payload of a NaN give identical outputs — and the finite rows
    beside them keep the bits they have without such neighbours.  The fp32 restatement on the same rows is deterministic in the payload too
    (ReLU maps NaN to 0; it returns finite actions where the reference returns NaN: DESIGN section 9)."""
    w = _nets(golden_dir)[net]
    ob, hh, mm = S.ordinary_rows(8, 99)
    rows = S.nonfinite_rows(ob[0], hh[0])
    obs = np.concatenate([ob, np.stack([r[1] for r in rows])])
    h = np.concatenate([hh, np.stack([r[2] for r in rows])])
    m = np.concatenate([mm, np.array([r[3] for r in rows], np.float32)])
    a, ho = ActorOracle(w, 'i8').forward(obs, h, m)
    assert np.isnan(a[8:]).all() and np.isnan(ho[8:]).all()
    a0, h0 = ActorOracle(w, 'i8').forward(ob, hh, mm)
    assert S.same_bits(a[:8], a0) and S.same_bits(ho[:8], h0) and np.isfinite(a0).all()
    f = ActorOracle(w, 'fp32')
    a32, h32 = f.forward(obs, h, m)
    by_name = {r[0]: i + 8 for i, r in enumerate(rows)}
    for where in ('obs[3]', 'h[37]', 'h[:]'):
        for mask in (0, 1):
            i, j, k = (by_name[f'{where}={v},mask={mask}'] for v in ('+nan', '-nan', 'nan_payload'))
            assert S.same_bits(a32[i], a32[j]) and S.same_bits(a32[i], a32[k]) and S.same_bits(h32[i], h32[j]) and S.same_bits(h32[i], h32[k]), (where, mask)
