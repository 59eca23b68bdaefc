"""Inputs and host-side classification for the controller's block-fixed-point numerics (oracle/f16_actor_i8.inc, csrc/np_actor_i8.h):
edge rows of the recurrent state built class by class, observation rows found by a host scan, synthetic networks whose weights sit on the
packer's edges, non-finite rows.  No assertions here (tests/test_actor_i8_spec_cpu.py, tests/test_gpu_actor_i8_edges.py hold them); the
role tests/math_spec.py and tests/noise_spec.py play for their pieces.

Conventions of the spec: exponent(b) = e with |b| < 2^e (exponent field - 126), clamped at -100; q = round-half-even(x 2^(22 - ex));
balanced limbs = bytes of (q + 0x808080) ^ 0x808080; lane layout f = 32 w + 8 g + 4 h + t."""
import numpy as np

XBITS, WBITS, CLAMP = 22, 29, -100
F32 = np.float32
E_LIST = (-100, -99, -30, 0, 1, 126, 127)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def bits(x):
    return f32(x).view(np.uint32)


def exponent(b):
    """The spec's row exponent of b >= 0 (array): field - 126, clamped at -100 (an infinity or a NaN: 129)."""
    return np.maximum(((bits(b) >> 23) & 255).astype(np.int64) - 126, CLAMP)


def pow2(e):
    return np.ldexp(1.0, np.asarray(e, np.int64))          # float64, exact


def next_f32(x, steps):
    """x moved by `steps` units in the last place (x > 0, finite)."""
    return (bits(x).astype(np.int64) + steps).astype(np.uint32).view(np.float32).reshape(np.shape(x))[()]


def exact_q(x, ex):
    """(round-half-even(x 2^(22 - ex)) as int64, is-a-tie mask): x float32, the product exact in float64."""
    s = f32(x).astype(np.float64) * pow2(XBITS - np.asarray(ex, np.int64))
    fl = np.floor(s)
    return np.rint(s).astype(np.int64), (s - fl) == 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# the recurrent state: quantised directly with eh = exponent(max |h mask|), so every class is constructed
# ---------------------------------------------------------------------------------------------------------------------------------
def classify_h(hm):
    """Masked recurrent-state rows [n, 128] -> list of sets of class names per row (finite rows only; a non-finite row: {'nonfinite'})."""
    hm = f32(hm)
    out = []
    for row in hm:
        c = set()
        if not np.isfinite(row).all():
            out.append({'nonfinite'})
            continue
        m = np.abs(row).max()
        if m == 0:
            out.append({'zero_row'})
            continue
        eh = int(exponent(F32(m))[0])
        mb = int(bits(F32(m))[0])
        if (mb & 0x7FFFFF) == 0:
            c.add('rowmax_pow2')
        if (mb & 0x7FFFFF) == 0x7FFFFF:
            c.add('rowmax_pow2_minus_ulp')
        if (mb & 0x7FFFFF) == 1:
            c.add('rowmax_pow2_plus_ulp')
        if ((mb >> 23) & 255) - 126 < CLAMP:
            c.add('exponent_clamped')
        if eh in (-100, -99):
            c.add('exponent_at_clamp')
        if eh >= 127:
            c.add('exponent_top')
        if m >= 2.9e38:
            c.add('huge_3e38')
        q, tie = exact_q(row, eh)
        if (np.abs(q) == 2 ** 22).any():
            c.add('q_top_2^22')
        k = np.floor(np.abs(f32(row).astype(np.float64)) * pow2(XBITS - eh)).astype(np.int64)
        if (tie & (k % 2 == 0) & (row > 0)).any():
            c.add('tie_even_pos')
        if (tie & (k % 2 == 1) & (row > 0)).any():
            c.add('tie_odd_pos')
        if (tie & (k % 2 == 0) & (row < 0)).any():
            c.add('tie_even_neg')
        if (tie & (k % 2 == 1) & (row < 0)).any():
            c.add('tie_odd_neg')
        for sign, name in ((1, 'pos'), (-1, 'neg')):
            qq = q[(q * sign) > 0] & 0xFFFFFF             # two's complement, as the kernel splits it: a byte >= 0x80 carries into the next limb
            b0, b1 = qq & 255, (qq >> 8) & 255
            for val, vn in ((0x7F, '7f'), (0x80, '80')):
                if (b0 == val).any():
                    c.add(f'limb0_{vn}_{name}')
                if (b1 == val).any():
                    c.add(f'limb1_{vn}_{name}')
            if ((b0 == 0x80) & (b1 == 0x80)).any() or ((b0 == 0x80) & (b1 == 0x7F)).any():
                c.add(f'limb01_carry_{name}')
        nz = np.nonzero(row)[0]
        if nz.size == 1:
            f = int(nz[0])
            c.add(f'single_w{f >> 5}g{(f >> 3) & 3}h{(f >> 2) & 1}')
        out.append(c)
    return out


H_CLASSES = (['zero_row', 'rowmax_pow2', 'rowmax_pow2_minus_ulp', 'rowmax_pow2_plus_ulp', 'exponent_clamped', 'exponent_at_clamp', 'exponent_top',
              'huge_3e38', 'q_top_2^22', 'tie_even_pos', 'tie_odd_pos', 'tie_even_neg', 'tie_odd_neg'] +
             [f'limb{b}_{v}_{s}' for b in (0, 1) for v in ('7f', '80') for s in ('pos', 'neg')] + ['limb01_carry_pos', 'limb01_carry_neg'] +
             [f'single_w{w}g{g}h{h}' for w in range(4) for g in range(4) for h in range(2)] + ['masked_out'])


def edge_h_rows(seed=11):
    """(h [R, 128] float32, mask [R] float32): every class of H_CLASSES constructed; classify_h(h * mask) says which row holds which."""
    rng = np.random.RandomState(seed)
    rows, masks = [], []

    def fill(m, top):
        """a row of random values below `top` (float32) in magnitude, element 0..: the given special values"""
        r = (rng.uniform(-0.9, 0.9, 128) * np.float64(top)).astype(np.float32)
        r[:len(m)] = m
        p = rng.permutation(128)
        return r[p]

    for e in E_LIST:
        p = F32(np.ldexp(1.0, e))
        below, above = next_f32(p, -1), next_f32(p, 1)
        rows += [fill([p], below), fill([-below], below), fill([above, -p], p)]
        masks += [1, 1, 1]
    for eh in (0, -7, 5):                                   # ties and limb carries at a fixed row exponent: row maximum 1.5 2^(eh - 1)
        top = F32(1.5 * 2.0 ** (eh - 1))
        unit = 2.0 ** (eh - XBITS)
        ks = np.array([0, 1, 2, 3, 126, 127, 128, 255, 256, 32767, 32768, 2 ** 21, 2 ** 21 + 1, 2 ** 22 - 2, 2 ** 22 - 1], np.float64)
        ties = np.concatenate([(ks + 0.5) * unit, -(ks + 0.5) * unit])
        rows.append(fill([top] + list(ties.astype(np.float32)), 0.0))
        qs = []
        for b2 in (0, 1, 0x3F):
            for b1 in (0, 0x7F, 0x80, 0x81):
                for b0 in (0x7E, 0x7F, 0x80, 0x81):
                    qs.append((b2 << 16) | (b1 << 8) | b0)
        qs = np.array(qs, np.float64)
        rows.append(fill([top] + list((qs * unit).astype(np.float32)), 0.0))
        rows.append(fill([-top] + list((-qs * unit).astype(np.float32)), 0.0))
        masks += [1, 1, 1]
    rows.append(np.zeros(128, np.float32)); masks.append(1)
    rows.append(fill([F32(1e30)], 1e30)); masks.append(0)                        # zeroed by its mask
    rows.append(fill([], 1e-39)); masks.append(1)                                # denormals only: exponent clamped
    rows.append(fill([F32(2.0 ** -110)], 2.0 ** -111)); masks.append(1)          # tiny normal numbers: exponent clamped
    rows.append(fill([F32(3e38), F32(-3e38)], 3e38)); masks.append(1)
    k = 0
    for w in range(4):
        for g in range(4):
            for h in range(2):
                r = np.zeros(128, np.float32)
                r[32 * w + 8 * g + 4 * h + (k & 3)] = F32((-1) ** k * (0.3 + 0.01 * k))
                rows.append(r); masks.append(1)
                k += 1
    return f32(np.stack(rows)), f32(masks)


def h_classes_of(h, mask):
    cl = classify_h(f32(h) * f32(mask).reshape(-1, 1))
    for c, m, row in zip(cl, f32(mask).reshape(-1), f32(h)):
        if m == 0 and np.abs(row).max() > 1:
            c.add('masked_out')
    return cl


# ---------------------------------------------------------------------------------------------------------------------------------
# observations: they reach the quantiser only through LayerNorm(22), so rows are FOUND (emulation in numpy fp32, bit-checked against the export)
# ---------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays through float64 (a b exact; one double rounding in 2^29 sums may differ: the CPU test bit-checks the result)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ln0_emulate(w, obs):
    """LayerNorm(22) of f16_actor_i8.inc in numpy float32: (y [n, 22], B [n] the bound, ex [n])."""
    x = f32(obs)
    g, b = f32(w[0:22]), f32(w[22:44])
    with np.errstate(all='ignore'):
        total = np.zeros(x.shape[0], np.float32)
        for j in range(22):
            total = total + x[:, j]
        mean = total * F32(1.0 / 22.0)
        d = x - mean[:, None]
        qt = np.zeros(x.shape[0], np.float32)
        for j in range(22):
            qt = _fma32(d[:, j], d[:, j], qt)
        var = qt * F32(1.0 / 22.0)
        m = np.abs(d).max(1)
        rstd = F32(1.0) / np.sqrt(var + F32(1e-5))
        y = _fma32(d * rstd[:, None], np.broadcast_to(g, d.shape), np.broadcast_to(b, d.shape))
        B = _fma32(m * rstd, np.full_like(m, np.abs(g).max()), np.full_like(m, np.abs(b).max())) * F32(1.000001)
    return y, B, exponent(B)


def classify_obs(w, obs):
    """Finite observation rows -> list of sets of class names (through the emulation of LayerNorm 0 of network w)."""
    obs = f32(obs)
    y, B, ex = ln0_emulate(w, obs)
    q, tie = exact_q(y, ex[:, None])
    mant = bits(B) & 0x7FFFFF
    aq = q & 0xFFFFFF                                     # two's complement bytes: >= 0x80 carries into the next limb
    b0, b1 = aq & 255, (aq >> 8) & 255
    d0 = (obs == obs[:, :1]).all(1)
    out = []
    for i in range(obs.shape[0]):
        c = set()
        if not np.isfinite(obs[i]).all():
            out.append({'nonfinite'})
            continue
        if mant[i] <= 4:
            c.add('bound_at_or_above_pow2')
        if mant[i] >= 0x7FFFFF - 3:
            c.add('bound_below_pow2')
        if tie[i].any():
            c.add('obs_tie')
        for l, bb in ((0, b0[i]), (1, b1[i])):
            if (bb == 0x7F).any():
                c.add(f'obs_limb{l}_7f')
            if (bb == 0x80).any():
                c.add(f'obs_limb{l}_80')
        if ((b0[i] == 0x80) & ((b1[i] == 0x80) | (b1[i] == 0x7F))).any():
            c.add('obs_limb01_carry')
        if d0[i] and np.all(y[i] == f32(w[22:44])):
            c.add('obs_constant_row')
        a = np.abs(obs[i]).max()
        if a >= 2.9e38:
            c.add('obs_huge_3e38')
        elif a >= 9e19:
            c.add('obs_huge_1e20')
        out.append(c)
    return out


OBS_CLASSES = ['bound_at_or_above_pow2', 'bound_below_pow2', 'obs_tie', 'obs_limb0_7f', 'obs_limb0_80', 'obs_limb1_7f', 'obs_limb1_80', 'obs_limb01_carry', 'obs_constant_row',
               'obs_huge_1e20', 'obs_huge_3e38']


def _bound_crossings(w, base, target):
    """Scale factors s (float32, per base row) at which the LayerNorm bound of s * base crosses the power of two `target`: bisection over the
    float32 bit patterns of s (the bound grows with s: the 1e-5 under the root matters less and less).  Returns rows on both sides."""
    lo = np.full(base.shape[0], int(bits(F32(1e-4))[0]), np.int64)
    hi = np.full(base.shape[0], int(bits(F32(1e4))[0]), np.int64)

    def B(sb):
        return ln0_emulate(w, base * sb.astype(np.uint32).view(np.float32)[:, None])[1]
    ok = (B(lo) < target) & (B(hi) >= target)
    for _ in range(34):
        mid = (lo + hi) // 2
        up = B(mid) >= target
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    rows = []
    for sb in (lo, hi, lo - 1, hi + 1):
        rows.append((base * sb.astype(np.uint32).view(np.float32)[:, None])[ok])
    return f32(np.concatenate(rows))


_EDGE_OBS = {}


def edge_obs_rows(w, seed=5, scan=200_000):
    """Cached per LayerNorm 0 (the scan is the same for every caller): see _edge_obs_rows."""
    key = (f32(w[0:44]).tobytes(), seed, scan)
    if key not in _EDGE_OBS:
        _EDGE_OBS[key] = _edge_obs_rows(w, seed, scan)
    return _EDGE_OBS[key].copy()


def _edge_obs_rows(w, seed, scan):
    """Observation rows [R, 22] that reach every class of OBS_CLASSES under network w's LayerNorm 0 (at most three rows per class), found by
    scanning `scan` random rows and the structured candidates; classify_obs(w, rows) says which row holds which."""
    rng = np.random.RandomState(seed)
    cand = [(rng.normal(0, 1, (scan, 22)) * rng.uniform(0.1, 30, (1, 22))).astype(np.float32)]
    base = rng.normal(0, 1, (64, 22)).astype(np.float32)
    gmax, bmax = float(np.abs(w[0:22]).max()), float(np.abs(w[22:44]).max())
    for k in range(-3, 6):
        if bmax < 2.0 ** k < bmax + 4.0 * gmax:
            cand.append(_bound_crossings(w, base, F32(2.0 ** k)))
    const = np.stack([np.full(22, v, np.float32) for v in (0.0, 0.5, 1.0, -3.0, 1e20)])
    huge = np.tile(rng.normal(0, 1, (4, 22)).astype(np.float32), (1, 1))
    huge[0, 5], huge[1, 17], huge[2, 0], huge[3, 21] = 1e20, -1e20, 3e38, -3e38
    cand += [const, huge]
    cand = f32(np.concatenate(cand))
    cl = classify_obs(w, cand)
    keep, count = [], {c: 0 for c in OBS_CLASSES}
    order = list(range(scan, cand.shape[0])) + list(range(scan))          # the structured rows first
    for i in order:
        new = [c for c in cl[i] if c in count and count[c] < 3]
        if new:
            keep.append(i)
            for c in cl[i]:
                if c in count:
                    count[c] += 1
        if all(v >= 3 for v in count.values()):
            break
    return cand[keep]


# ---------------------------------------------------------------------------------------------------------------------------------
# synthetic networks on the packer's edges (state dicts for neuralplane_amd.actor.pack_ppo_actor, the shipped shapes)
# ---------------------------------------------------------------------------------------------------------------------------------
LINEARS = ['base.mlp.fc.0', 'base.mlp.fc.3', 'rnn.gru.weight_ih_l0', 'rnn.gru.weight_hh_l0', 'act.mlp.fc.0', 'act.mlp.fc.3']
NORMS = ['base.feature_norm', 'base.mlp.fc.2', 'base.mlp.fc.5', 'rnn.norm', 'act.mlp.fc.2', 'act.mlp.fc.5']


def _wkey(name):
    return name if name.startswith('rnn.gru') else name + '.weight'


def _bkey(name):
    return name.replace('weight', 'bias') if name.startswith('rnn.gru') else name + '.bias'


def _random_sd(seed, scale=1.0):
    rng = np.random.RandomState(seed)
    sd = {}
    for name, (o, i) in zip(LINEARS, ((128, 22), (128, 128), (384, 128), (384, 128), (128, 128), (128, 128))):
        sd[_wkey(name)], sd[_bkey(name)] = scale * rng.normal(size=(o, i)) / np.sqrt(i), 0.1 * rng.normal(size=o)
    for name in NORMS:
        n = 22 if name == 'base.feature_norm' else 128
        sd[name + '.weight'], sd[name + '.bias'] = (1 + 0.3 * rng.normal(size=n)) * rng.choice([-1.0, 1.0], n), 0.2 * rng.normal(size=n)
    sd['act.action_out.mu_net.fc.0.weight'], sd['act.action_out.mu_net.fc.0.bias'] = 0.2 * rng.normal(size=(4, 128)), 0.1 * rng.normal(size=4)
    return {k: np.asarray(v, np.float32) for k, v in sd.items()}


WEIGHT_WQ = [0x7F, 0x80, 0x81, 0x7F00, 0x8000, 0x7F80, 0x8080, 0x7F0000, 0x800000, 0x808080, 0x7F7F7F, 0x807F80]      # limb carries: all < 2^24, exact in float32


def weight_edges_net(seed=21):
    """Rows 0..5 of every quantised Linear on the packer's edges: maximum 2^-3; 2^-3 - ulp; all zero (ew clamped); ties of rint(W 2^(29 - ew));
    the weight-limb carries; wq = +-2^28 and its neighbours.  Biases +-1e30 and 0 on rows 6..8; LayerNorm terms of mixed sign."""
    sd = _random_sd(seed)
    for name in LINEARS:
        W, b = sd[_wkey(name)], sd[_bkey(name)]
        k = W.shape[1]
        p = F32(2.0 ** -3)
        W[0] = np.clip(W[0], -0.1, 0.1); W[0, 1] = p                                  # ew = -2, wq = 2^28
        W[1] = np.clip(W[1], -0.1, 0.1); W[1, 2] = -next_f32(p, -1)                    # ew = -3, wq = -(2^29 - 32)
        W[2] = 0
        ew = -2
        unit = 2.0 ** (ew - WBITS)
        W[3] = 0; W[3, 0] = F32(0.75 * 2.0 ** ew)
        ks = np.array([0, 1, 2, 3, 127, 128, 2 ** 22, 2 ** 22 + 1, 2 ** 23 - 2, 2 ** 23 - 1], np.float64)
        t = np.concatenate([(ks + 0.5) * unit, -(ks + 0.5) * unit]).astype(np.float32)
        W[3, 1:1 + t.size] = t
        W[4] = 0; W[4, 0] = F32(0.75 * 2.0 ** ew)
        c = np.array(WEIGHT_WQ[:(k - 2) // 2], np.float64) * unit
        W[4, 1:1 + c.size] = c.astype(np.float32); W[4, 1 + c.size:1 + 2 * c.size] = (-c).astype(np.float32)
        W[5] = np.clip(W[5], -0.1, 0.1)
        W[5, 0], W[5, 1], W[5, 2], W[5, 3] = F32(2.0 ** (ew - 1)), -F32(2.0 ** (ew - 1)), F32((2.0 ** 28 - 16) * unit), -F32((2.0 ** 28 - 16) * unit)
        b[6], b[7], b[8] = 1e30, -1e30, 0.0
    return sd


def flat_norms_net(seed=22):
    """LayerNorm terms that are zero or tiny: gamma = beta = 0 (bound 0: the exponent clamp, every quantised value 0), tiny gamma, tiny beta."""
    sd = _random_sd(seed)
    tiny = F32(2.0 ** -120)
    for j, name in enumerate(NORMS):
        g, b = sd[name + '.weight'], sd[name + '.bias']
        if j in (0, 3):
            g[:], b[:] = 0, 0
        elif j in (1, 4):
            g[:], b[:] = np.sign(g) * tiny, 0
        else:
            g[:], b[:] = 0, np.sign(b) * tiny
    return sd


def steep_norms_net(seed=23):
    """LayerNorm gammas of 2^100 (the observation's) and 2^60, mixed sign, the Linear behind each scaled back by as much: row exponents
    up to 104.  (The epilogue's u * 2^(ex - 17) needs ex < 106 to stay finite whatever the weights: DESIGN section 9.)"""
    sd = _random_sd(seed)
    follow = {0: [0], 1: [1], 2: [2], 3: [4], 4: [5]}
    for j, name in enumerate(NORMS[:5]):
        s = 100 if j == 0 else 60
        sd[name + '.weight'] *= F32(2.0 ** s)
        sd[name + '.bias'] *= F32(2.0 ** (s - 3))
        for L in follow[j]:
            sd[_wkey(LINEARS[L])] *= F32(2.0 ** -(s - 8 if j == 0 else s))
    return sd


def synthetic_nets():
    return {'weight_edges': weight_edges_net(), 'flat_norms': flat_norms_net(), 'steep_norms': steep_norms_net()}


def classify_weights(W):
    """A Linear's weight matrix [n_out, n_in] float32 -> set of packer classes its rows reach (exact arithmetic)."""
    W = f32(W)
    c = set()
    for row in W:
        m = np.abs(row).max()
        ew = int(exponent(F32(m))[0])
        mb = int(bits(F32(m))[0])
        if m == 0:
            c.add('w_row_zero')
            continue
        if (mb & 0x7FFFFF) == 0:
            c.add('w_rowmax_pow2')
        if (mb & 0x7FFFFF) == 0x7FFFFF:
            c.add('w_rowmax_pow2_minus_ulp')
        s = row.astype(np.float64) * pow2(WBITS - ew)
        if ((s - np.floor(s)) == 0.5).any():
            c.add('w_tie')
        wq = np.abs(np.rint(s).astype(np.int64))
        for l in range(3):
            byte = (wq >> (8 * l)) & 255
            if (byte == 0x80).any() and (byte == 0x7F).any():
                c.add(f'w_limb{l}_carry')
        if (wq == 2 ** 28).any():
            c.add('w_wq_2^28')
        if (wq == 2 ** 29 - 32).any():
            c.add('w_wq_top')
    return c


W_CLASSES = ['w_row_zero', 'w_rowmax_pow2', 'w_rowmax_pow2_minus_ulp', 'w_tie', 'w_limb0_carry', 'w_limb1_carry', 'w_limb2_carry', 'w_wq_2^28', 'w_wq_top']


def same_bits(a, b):
    """Bit for bit, -0 != +0; NaN == NaN whatever its sign and payload."""
    a, b = f32(a), f32(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------------------------
# non-finite rows
# ---------------------------------------------------------------------------------------------------------------------------------
def nan32(sign=0, payload=0x400000):
    return np.array([(sign << 31) | 0x7F800000 | payload], np.uint32).view(np.float32)[0]


NONFINITE_VALUES = {'+inf': F32(np.inf), '-inf': F32(-np.inf), '+nan': nan32(0), '-nan': nan32(1), 'nan_payload': nan32(0, 0x2ABCDE), '-snan_payload': nan32(1, 0x012345)}


def nonfinite_rows(obs0, h0):
    """Variants of one ordinary row (obs0 [22], h0 [128]): list of (name, obs, h, mask).  The contract: every one comes out all-NaN, whatever the
    sign or payload of its NaN."""
    rows = []
    for name, v in NONFINITE_VALUES.items():
        for mask in (1.0, 0.0):
            o = obs0.copy(); o[3] = v
            rows.append((f'obs[3]={name},mask={int(mask)}', o, h0.copy(), mask))
            h = h0.copy(); h[37] = v
            rows.append((f'h[37]={name},mask={int(mask)}', obs0.copy(), h, mask))
            rows.append((f'h[:]={name},mask={int(mask)}', obs0.copy(), np.full(128, v, np.float32), mask))
    o = obs0.copy(); o[2], o[9] = np.inf, -np.inf
    rows.append(('obs=+inf,-inf', o, h0.copy(), 1.0))
    o = obs0.copy(); o[2], o[9] = np.inf, np.inf
    rows.append(('obs=+inf,+inf', o, h0.copy(), 1.0))
    h = h0.copy(); h[0], h[127] = np.inf, -np.inf
    rows.append(('h=+inf,-inf', obs0.copy(), h, 1.0))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# batches: edge rows interleaved with ordinary rows
# ---------------------------------------------------------------------------------------------------------------------------------
def ordinary_rows(n, seed):
    rng = np.random.RandomState(seed)
    obs = (rng.normal(0, 1, (n, 22)) * rng.uniform(0.1, 30, (1, 22))).astype(np.float32)
    return obs, rng.normal(0, 0.5, (n, 128)).astype(np.float32), np.ones(n, np.float32)


def edge_slots(n):
    """Positions of a batch of n that take edge rows: every second row, and lanes 0 and 31 of every 32-row tile."""
    return [i for i in range(n) if i % 2 == 0 or i % 32 == 31]


def batches(n, edge_obs, edge_h, edge_mask, extra=(), seed=0):
    """Batches of n rows holding every edge row once: [(obs, h, mask, kinds)], kinds[i] = ('h', j) | ('obs', j) | ('extra', j) | None.
    An edge h row meets an ordinary observation and the other way round; `extra` = [(name, obs, h, mask)] rows placed as they are."""
    todo = [('h', j) for j in range(edge_h.shape[0])] + [('obs', j) for j in range(edge_obs.shape[0])] + [('extra', j) for j in range(len(extra))]
    slots = edge_slots(n)
    out = []
    for b0 in range(0, len(todo), len(slots)):
        obs, h, mask = ordinary_rows(n, seed + 1000 * n + b0)
        kinds = [None] * n
        for s, (kind, j) in zip(slots, todo[b0:b0 + len(slots)]):
            kinds[s] = (kind, j)
            if kind == 'h':
                h[s], mask[s] = edge_h[j], edge_mask[j]
            elif kind == 'obs':
                obs[s] = edge_obs[j]
            else:
                _, obs[s], h[s], mask[s] = extra[j]
        out.append((obs, h, mask, kinds))
    return out
