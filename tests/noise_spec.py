"""Shared pieces of the observation-noise tests (tests/test_noise_spec_cpu.py, tests/test_gpu_noise_edges.py): the fp64 reference
of the generator on its whole index grid, and the scan for rows whose draws sit on an edge of the index range.

TEST INFRASTRUCTURE ONLY.  The reference everywhere is numpy fp64: sqrt(-2 log u), cos, sin.
"""
import functools

import numpy as np

from oracle import f16_oracle as fo

NBITS = 21
NIDX = 1 << NBITS                     # values of K1 and of K2
NBASE = 1 << 18                       # base angles; bits 18, 19, 20 of K2: swap, sign of cos, sign of sin
SWAP, NEG_C, NEG_S = 1 << 18, 1 << 19, 1 << 20


@functools.lru_cache(maxsize=None)
def radius_tables():
    """All 2^21 K1: (u, w, r) float32 of the oracle and (u64, w64, r64) of the fp64 reference."""
    k = np.arange(NIDX, dtype=np.uint32)
    u, w, r = fo.noise_radius(k)
    u64 = (k.astype(np.float64) + 0.5) / NIDX
    w64 = -2.0 * np.log(u64)
    out = (u, w, r, u64, w64, np.sqrt(w64))
    for a in out:
        a.setflags(write=False)
    return out


def direction_ref(k2):
    """fp64 (cos, sin) of the direction index: angle ((K2 & 0x3FFFF) + 1/2) (pi/4) / 2^18, then swap and signs."""
    k2 = np.asarray(k2, dtype=np.uint32)
    th = ((k2 & (NBASE - 1)).astype(np.float64) + 0.5) * (np.pi / 4) / NBASE
    c, s = np.cos(th), np.sin(th)
    sw = (k2 & SWAP) != 0
    a, b = np.where(sw, s, c), np.where(sw, c, s)
    return np.where((k2 & NEG_C) != 0, -a, a), np.where((k2 & NEG_S) != 0, -b, b)


@functools.lru_cache(maxsize=None)
def direction_tables():
    """All 2^21 K2: (cs, sn) float32 of the oracle and (c64, s64) of the fp64 reference."""
    k = np.arange(NIDX, dtype=np.uint32)
    cs, sn = fo.noise_direction(k)
    c64, s64 = direction_ref(k)
    out = (cs, sn, c64, s64)
    for a in out:
        a.setflags(write=False)
    return out


def argmax_error_indices():
    """K1 of the largest relative error of w = neg2ln_spec(u) and of r = sqrt_spec(w) against fp64, over all 2^21 indices."""
    _, w, r, _, w64, r64 = radius_tables()
    return (int(np.argmax(np.abs(w.astype(np.float64) - w64) / w64)), int(np.argmax(np.abs(r.astype(np.float64) - r64) / r64)))


def seam_indices():
    """K1 next to the exponent / mantissa seams of neg2ln_spec: u = sqrt(1/2) 2^e, e = 0 .. -3."""
    return [int(np.floor(np.sqrt(0.5) * 2.0 ** e * NIDX - 0.5)) for e in range(0, -4, -1)]


# ---- edge rows ---------------------------------------------------------------------------------------------------------------
GROUPS = {'top_packed_0_7': list(range(8)), 'low_packed_8_9': [8, 9], 'low_scalar_10': [10]}


def _near(k, centres, d=4):
    m = np.zeros(k.shape, bool)
    for c in centres:
        m |= np.abs(k.astype(np.int64) - c) <= d
    return m


def edge_classes(k1, k2):
    """{class name: (mask[n, 11], which index array it speaks of)} for index arrays [n, 11]."""
    base = k2 & (NBASE - 1)
    return {
        'k1_lt_8': (k1 < 8, k1),
        'k1_top_8': (k1 >= NIDX - 8, k1),
        'k1_log_seam': (_near(k1, seam_indices()), k1),
        'k1_argmax_error': (_near(k1, argmax_error_indices()), k1),
        'angle_lt_8': (base < 8, k2),
        'angle_top_8': (base >= NBASE - 8, k2),
    }


CENTRES = {'k1_log_seam': seam_indices, 'k1_argmax_error': argmax_error_indices}     # classes that pool several index neighbourhoods


def _centre(cname, K):
    """Which neighbourhood of a pooled class the index K belongs to (0 for the other classes)."""
    if cname not in CENTRES:
        return 0
    c = CENTRES[cname]()
    return int(np.argmin([abs(K - x) for x in c]))


def find_edge_rows(seed, call_idx, row_start, nrows, chunk=500_000, keep=3):
    """Scan global rows row_start .. row_start + nrows - 1 of (seed, call_idx) and keep up to `keep` rows per (class, group) cell in
    which a pair of that group draws an index of that class.  The seam class pools four neighbourhoods and the arg-max class two:
    a cell takes rows of neighbourhoods it does not hold yet first.  Returns a list of {class, group, row, pair, K, centre}."""
    cand = {}
    ncentres = {c: len(CENTRES[c]()) if c in CENTRES else 1 for c in edge_classes(*fo.noise_indices_rows(seed, call_idx, 0, 1))}

    def full(cell):
        got = cand.get(cell, [])
        return len(got) >= keep and len({h['centre'] for h in got}) >= min(keep, ncentres[cell[0]])

    for r0 in range(row_start, row_start + nrows, chunk):
        if cand and all(full((c, g)) for c in ncentres for g in GROUPS):
            break
        n = min(chunk, row_start + nrows - r0)
        k1, k2 = fo.noise_indices_rows(seed, call_idx, r0, n)
        for cname, (mask, k) in edge_classes(k1, k2).items():
            for gname, pairs in GROUPS.items():
                cell = (cname, gname)
                if full(cell):
                    continue
                rows, cols = np.nonzero(mask[:, pairs])
                for i, j in zip(rows.tolist()[:256], cols.tolist()[:256]):
                    K = int(k[i, pairs[j]])
                    cand.setdefault(cell, []).append({'class': cname, 'group': gname, 'row': r0 + i, 'pair': pairs[j], 'K': K,
                                                      'centre': _centre(cname, K)})
    hits = []
    for cell, got in cand.items():
        first = {}
        for h in got:                                  # the first row of every neighbourhood, then the earliest of the rest
            first.setdefault(h['centre'], h)
        chosen = list(first.values())[:keep]
        chosen += [h for h in got if not any(h is c for c in chosen)][:keep - len(chosen)]
        hits.extend(sorted(chosen, key=lambda h: h['row']))
    return hits
