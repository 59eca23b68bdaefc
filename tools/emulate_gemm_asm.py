#!/usr/bin/env python3
"""Bit-exact CPU emulation of the generated GEMM-order net bodies (tools/gen_mlp_asm.py::BodyGemm, np_mlp_asm_gemm.inc).

Executes the instruction TEXT of one net body — the weight stream (s_load_dwordx16 into the SGPR buffers, retired at the s_waitcnt
or at once), v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32 with op_sel / op_sel_hi / clamp, v_mul_f32 / v_fmac_f32 / v_add_f32 — in
fp32 arithmetic with a correctly rounded fused multiply-add, vectorised over the input rows, on a record in the KBLOB_GEMM layout
(np_nets.h::gemm_record_len).  The check on operand order and record addressing that needs no GPU: tests/test_gemm_order_cpu.py
compares it bit for bit with the CPU oracle's bias-last mode.

    python tools/emulate_gemm_asm.py      # self-check on random nets of every shape against a plain restatement of the contract
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_mlp_asm as G  # noqa: E402

ACT_SHIFT = 40


def fma32(a, b, c):
    """RN_fp32(a * b + c) for float32 arrays: the product is exact in fp64, the sum is rounded to odd in fp64 (TwoSum), and a round-to-odd
    53-bit value rounds to 24 bits as the exact sum does."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        toward = np.where((err > 0) == (s > 0), 1, -1)   # the exact sum lies further from / nearer to zero than s
        toward = np.where(s == 0, 0, toward)
        s2 = (bits + np.where(fix, toward, 0)).view(np.float64)
        return s2.astype(np.float32)


def pack_gemm(layers, out_layer, out_std, out_mean, shape):
    """one record in the KBLOB_GEMM layout; parameters scaled as np_pack_kblob scales them (first layer's weights and hidden biases
    x 2^-ACT_SHIFT, output weights x 2^+ACT_SHIFT).  layers: [(W[out][in], b[out])], out_layer: (w[in], b)"""
    rec = []
    for l, (W, b) in enumerate(layers):
        out, inn = W.shape
        row = G.pad2(out)
        for k in range(inn):
            col = np.zeros(row, np.float32)
            col[:out] = np.ldexp(W[:, k], -ACT_SHIFT) if l == 0 else W[:, k]
            rec += list(col)
        col = np.zeros(row, np.float32)
        col[:out] = np.ldexp(b, -ACT_SHIFT)
        rec += list(col)
    w, b = out_layer
    col = np.zeros(G.pad2(len(w)), np.float32)
    col[:len(w)] = np.ldexp(np.asarray(w, np.float32), ACT_SHIFT)
    rec += list(col) + [np.float32(b), np.float32(0.0), np.float32(out_std), np.float32(out_mean)]
    n = G.record_len(*shape)
    assert len(rec) <= n
    return np.array(rec + [0.0] * (n - len(rec)), np.float32)


def run_body(shape, record, x, parity=0, land_at_wait=True):
    """x: float32[rows][IN] normalised inputs -> float32[rows], the value the body leaves in v126 (the net output)"""
    IN = shape[0]
    x = np.asarray(x, np.float32)
    rows = x.shape[0]
    blob = np.concatenate([record, np.zeros(2 * G.GROUP, np.float32)])   # the body prefetches one group past the record
    V = np.zeros((256, rows), np.float32)
    for k in range(IN):
        V[G.V_X + 2 * k] = x[:, k]
    SF = np.full(128, np.nan, np.float32)
    # prologue of the class / phase functions: the first group into the first CPG buffers (buffer parity as the body was generated for)
    for c in range(G.CPG):
        b = G.S_W0 + 16 * ((c + G.CPG * parity) % G.NBUF)
        SF[b:b + 16] = blob[16 * c:16 * c + 16]
    pending = []

    def src(tok, half):
        m = re.match(r's\[(\d+):', tok)
        if m:
            return np.float32(SF[int(m.group(1)) + half])
        m = re.match(r'v\[(\d+):', tok)
        if m:
            return V[int(m.group(1)) + half]
        m = re.match(r's(\d+)$', tok)
        if m:
            return np.float32(SF[int(m.group(1))])
        m = re.match(r'v(\d+)$', tok)
        assert m, tok
        return V[int(m.group(1))]

    def clamp(r, on):
        if not on:
            return r
        with np.errstate(invalid='ignore'):
            return np.where(r > 0, np.minimum(r, np.float32(1.0)), np.float32(0.0)).astype(np.float32)   # NaN -> 0, -0 -> +0

    for ins in G.BodyGemm(shape, parity).build():
        op, _, rest = ins.partition(' ')
        if op == 's_waitcnt':
            for dst, off in pending:
                SF[dst:dst + 16] = blob[off:off + 16]
            pending = []
            continue
        if op == 's_load_dwordx16':
            m = re.match(r's\[(\d+):\d+\], s\[(\d+):\d+\], (0x[0-9a-f]+)', rest)
            dst, off = int(m.group(1)), int(m.group(3), 16) // 4
            assert int(m.group(2)) == G.S_BASE and off + 16 <= len(blob), ins
            if land_at_wait:
                pending.append((dst, off))
            else:
                SF[dst:dst + 16] = blob[off:off + 16]
            continue
        cl = ' clamp' in rest
        a = [t.strip() for t in re.split(r',\s*(?![^\[]*\])', re.split(r' op_sel| clamp', rest)[0])]
        if op.startswith('v_pk_'):
            m = re.search(r'op_sel:\[([\d,]+)\]', rest)
            lo = [int(t) for t in m.group(1).split(',')] if m else [0, 0, 0]
            m = re.search(r'op_sel_hi:\[([\d,]+)\]', rest)
            hi = [int(t) for t in m.group(1).split(',')] if m else [1, 1, 1]
            d = int(re.match(r'v\[(\d+):', a[0]).group(1))
            res = []
            for sel in (lo, hi):
                o = [src(t, sel[i]) for i, t in enumerate(a[1:])]
                if op == 'v_pk_mul_f32':
                    r = (np.float32(o[0]) * o[1]).astype(np.float32)
                elif op == 'v_pk_fma_f32':
                    r = fma32(np.broadcast_to(o[0], (rows,)), o[1], o[2])
                elif op == 'v_pk_add_f32':
                    r = (np.float32(o[0]) + o[1]).astype(np.float32)
                else:
                    raise ValueError('instruction not modelled: ' + ins)
                res.append(clamp(r, cl))
            V[d], V[d + 1] = res
            continue
        d = int(a[0][1:])
        if op == 'v_mul_f32':
            r = (src(a[1], 0) * src(a[2], 0)).astype(np.float32)
        elif op == 'v_add_f32':
            r = (src(a[1], 0) + src(a[2], 0)).astype(np.float32)
        elif op == 'v_fmac_f32':
            r = fma32(np.broadcast_to(src(a[1], 0), (rows,)), src(a[2], 0), V[d])
        else:
            raise ValueError('instruction not modelled: ' + ins)
        V[d] = clamp(r, cl)
    return V[G.V_Y].copy()


def contract(layers, out_layer, out_std, out_mean, x):
    """the arithmetic contract restated (unscaled parameters): acc = 0; fma chain, k ascending; + bias; plain ReLU; ONE output chain"""
    h = [np.asarray(x, np.float32)[:, k] for k in range(np.asarray(x).shape[1])]
    zero = np.zeros(len(h[0]), np.float32)
    for W, b in layers:
        nxt = []
        for j in range(W.shape[0]):
            acc = zero
            for k in range(W.shape[1]):
                acc = fma32(np.broadcast_to(W[j, k], acc.shape), h[k], acc)
            acc = (acc + b[j]).astype(np.float32)
            with np.errstate(invalid='ignore'):
                nxt.append(np.where(acc > 0, acc, np.float32(0.0)).astype(np.float32))
        h = nxt
    w, b = out_layer
    acc = zero
    for k in range(len(w)):
        acc = fma32(np.broadcast_to(np.float32(w[k]), acc.shape), h[k], acc)
    y = (acc + np.float32(b)).astype(np.float32)
    return ((y * np.float32(out_std)).astype(np.float32) + np.float32(out_mean)).astype(np.float32)


def random_net(rng, shape):
    IN, H1, H2, H3 = shape
    layers, prev = [], IN
    for h in [H1, H2] + ([H3] if H3 else []):
        layers.append((rng.randn(h, prev).astype(np.float32) * np.float32(0.4), rng.randn(h).astype(np.float32) * np.float32(0.2)))
        prev = h
    return layers, (rng.randn(prev).astype(np.float32) * np.float32(0.4), np.float32(rng.randn() * 0.1)), np.float32(1.7), np.float32(-0.3)


def self_check():
    rng = np.random.RandomState(0)
    bad = []
    for shape in G.SHAPES:
        layers, out_layer, sd, mu = random_net(rng, shape)
        rec = pack_gemm(layers, out_layer, sd, mu, shape)
        x = rng.randn(200, shape[0]).astype(np.float32)
        want = contract(layers, out_layer, sd, mu, x)
        for parity in (0, 1):
            for land in (True, False):
                got = run_body(shape, rec, x, parity, land)
                if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                    bad.append((shape, parity, land, int((got.view(np.uint32) != want.view(np.uint32)).sum())))
    return bad


if __name__ == '__main__':
    problems = self_check()
    print(problems if problems else 'BodyGemm: every shape, both buffer parities, loads landing at the wait and at once: bit-equal to the contract')
    sys.exit(1 if problems else 0)
