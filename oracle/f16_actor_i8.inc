/*
 * oracle/f16_actor_i8.inc — CPU restatement of the controller's SECOND numerics spec: "block fixed point" (round 5).  Same network as
 * f16_actor.inc (the reference's PPOActor in deterministic mode, algorithms/ppo/ppo_actor.py:38-64, configuration
 * envs/planning_env.py:18-29); what changes is HOW the six Linear layers with K <= 128 and N >= 128 are evaluated, and the order of
 * the LayerNorm sums.  TEST INFRASTRUCTURE ONLY, like the rest of oracle/.  (Included at the end of f16_oracle.c, after f16_actor.inc,
 * whose act_exp / act_sigmoid / act_tanh and weight offsets it shares.)
 *
 * The HIP kernels (neuralplane_amd/csrc/np_actor_i8.h) evaluate these layers on the i8 matrix pipe (v_mfma_i32_32x32x32_i8) and keep every
 * activation in that instruction's ACCUMULATOR layout: wave w (0..3) of a 32-aircraft tile owns features 32 w .. 32 w + 31 of a layer's
 * output, lane half h (0, 1) and accumulator register r = 4 g + t hold feature
 *         f = 32 w + 8 g + 4 h + t                                                         ("lane block" (w, h): 16 features, r ascending).
 * Integer arithmetic is exact, so the only things this file has to pin are the conversions and the floating-point steps around them:
 *
 *   LayerNorm(128)  per lane block s = sum of its 16 features in register order (sequential), total = blocks added in (w, h) order;
 *                   mean = total * (1/128); d = x - mean; q the same way with fmaf(d, d, q); var = qt * (1/128);
 *                   rstd = 1 / sqrtf(var + 1e-5f); y = fmaf(d * rstd, gamma, beta)      (nn.LayerNorm, eps 1e-5)
 *   LayerNorm(22)   the observation: one sequential chain over the 22 features, mean = total * (1/22 rounded to fp32)
 *   row exponent    of a LayerNorm output: from a BOUND that needs no reduction of its own — m = max |d| (exact, order-free) travels with
 *                   the variance sums — B = fmaf(m * rstd, max|gamma|, max|beta|) * 1.000001f, ex = exponent field of B - 126 (B < 2^ex),
 *                   clamped at -100; of the masked recurrent state: ex = exponent of max |h * mask|
 *   quantiser       q = bits(fmaf(x, 2^(22 - ex), 1.5 * 2^23)) - bits(1.5 * 2^23): round-half-even of x * 2^(22 - ex), |q| <= 2^22
 *                   (2^22 itself when |x| rounds up to the bound 2^ex, e.g. the recurrent state's largest element 2^eh - ulp);
 *                   three balanced signed 8-bit limbs: bytes 0..2 of (q + 0x808080) ^ 0x808080
 *   weights         (load time, per OUTPUT feature j) ew_j = exponent of max_k |W[j][k]|, wq = rint(W * 2^(29 - ew_j)) (round-half-even of the
 *                   exact product), four balanced limbs: bytes of (wq + 0x80808080) ^ 0x80808080
 *   Linear          the nine limb products of weight >= 2^16 as four exact int32 class sums over k
 *                       c0 = x2.w3   c1 = x2.w2 + x1.w3   c2 = x2.w1 + x1.w2 + x0.w3   c3 = x2.w0 + x1.w1 + x0.w2
 *                   (x1.w0 + x0.w1 and x0.w0 are dropped: < 2^-24 of the BOUND on the sum, K 2^(ex + ew) — not of a cancelled sum);
 *                   every |c| < 2^24 converts to fp32 exactly (both asserted: tests/test_actor_i8_spec_cpu.py);
 *                   u = fmaf(c0, 256, c1); u = fmaf(u, 256, c2); u = fmaf(u, 256, c3); y = fmaf(u * 2^(ex - 17), 2^(ew_j - 18), bias_j)
 *   head            Linear(128, 4): per lane block p = sequential fmaf(W[o][f], x[f], p) from 0 in register order; m_o = bias_o + the blocks
 *                   in (w, h) order; tanh as before
 *   GRU cell, exp   as f16_actor.inc
 *   non-finite rows a row whose observation bound B is an infinity, a NaN or >= 2^105 (row exponent 106: from there u * 2^(ex - 17) could overflow),
 *                   or whose masked recurrent state holds such a value, returns NaN in every
 *                   action (or value) and all 128 states; finite rows of the same tile are untouched (ai8_row)
 * Accuracy against the reference's recordings (tools/microbench/i8v2_numerics.py, tests): actions 5.2e-6 (open loop), closed loop over 150
 * inner steps states 4.1e-5 / recurrent state 1.8e-5 / actions 7.1e-6 — the same size as the fp32 spec's (3.9e-5 / 1.5e-5 / 5.0e-6).
 */
enum { AI8_XBITS = 22, AI8_WBITS = 29, AI8_MAGIC_BITS = 0x4B400000 };

static inline uint32_t ai8_bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
static inline float ai8_float(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
static inline int ai8_exponent(float b) {   /* e with |b| < 2^e, clamped below */
    const int e = (int)((ai8_bits(b) >> 23) & 255u) - 126;
    return e < -100 ? -100 : e;
}
enum { AI8_EX_RANGE = 106 };   /* a row exponent from here on (|x| >= 2^105, an infinity, a NaN): u * 2^(ex - 17) in ai8_dense could overflow whatever the weights */
static inline int ai8_nonfinite(float x) { return (int)((ai8_bits(x) >> 23) & 255u) - 126 >= AI8_EX_RANGE; }
static inline float ai8_pow2(int e) { return ai8_float((uint32_t)(e + 127) << 23); }   /* -126 <= e <= 127 */
static inline int ai8_feature(int blk, int r) { return 32 * (blk >> 1) + 8 * (r >> 2) + 4 * (blk & 1) + (r & 3); }

/* a quantised Linear layer: limbs[l][j][k] */
typedef struct {
    int n_in, n_out;
    int8_t *limb[4];
    int *ew;
    const float *bias;
} ai8_layer;

static int ai8_layer_init(ai8_layer *L, int n_in, int n_out, int ld, const float *wt /* k-major [n_in][ld] */, const float *bias) {
    L->n_in = n_in; L->n_out = n_out; L->bias = bias;
    L->ew = (int *)malloc(sizeof(int) * (size_t)n_out);
    for (int l = 0; l < 4; l++) L->limb[l] = (int8_t *)malloc((size_t)n_out * (size_t)n_in);
    if (!L->ew || !L->limb[0] || !L->limb[1] || !L->limb[2] || !L->limb[3]) return 1;
    for (int j = 0; j < n_out; j++) {
        float m = 0.0f;
        for (int k = 0; k < n_in; k++) { const float a = fabsf(wt[k * ld + j]); m = a > m ? a : m; }
        const int ew = ai8_exponent(m);
        L->ew[j] = ew;
        for (int k = 0; k < n_in; k++) {
            const int32_t q = (int32_t)rint(ldexp((double)wt[k * ld + j], AI8_WBITS - ew));   /* exact product, round-half-even */
            const uint32_t p = ((uint32_t)q + 0x80808080u) ^ 0x80808080u;
            for (int l = 0; l < 4; l++) L->limb[l][(size_t)j * n_in + k] = (int8_t)(uint8_t)(p >> (8 * l));
        }
    }
    return 0;
}
static void ai8_layer_free(ai8_layer *L) {
    for (int l = 0; l < 4; l++) free(L->limb[l]);
    free(L->ew);
}

/* the quantiser's two steps for one element: the magic-number sum, and the integer it holds */
static inline float ai8_qsum(float x, int ex) { return fmaf(x, ai8_pow2(AI8_XBITS - ex), ai8_float(AI8_MAGIC_BITS)); }
static inline int32_t ai8_q(float x, int ex) { return (int32_t)(ai8_bits(ai8_qsum(x, ex)) - (uint32_t)AI8_MAGIC_BITS); }

/* x[n_in] with row exponent ex -> three limb arrays */
static void ai8_quantise(int n, const float *x, int ex, int8_t *x0, int8_t *x1, int8_t *x2) {
    for (int k = 0; k < n; k++) {
        const int32_t q = ai8_q(x[k], ex);
        const uint32_t p = ((uint32_t)q + 0x808080u) ^ 0x808080u;
        x0[k] = (int8_t)(uint8_t)p; x1[k] = (int8_t)(uint8_t)(p >> 8); x2[k] = (int8_t)(uint8_t)(p >> 16);
    }
}

/* cs: 0, or [n_out][4] for the class sums c0..c3 */
static void ai8_dense(const ai8_layer *L, const int8_t *x0, const int8_t *x1, const int8_t *x2, int ex, float *y, int32_t *cs) {
    const int K = L->n_in;
    const float sa = ai8_pow2(ex - 17);
    for (int j = 0; j < L->n_out; j++) {
        const int8_t *w0 = L->limb[0] + (size_t)j * K, *w1 = L->limb[1] + (size_t)j * K, *w2 = L->limb[2] + (size_t)j * K, *w3 = L->limb[3] + (size_t)j * K;
        int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int k = 0; k < K; k++) {
            const int a0 = x0[k], a1 = x1[k], a2 = x2[k];
            c0 += a2 * w3[k];
            c1 += a2 * w2[k] + a1 * w3[k];
            c2 += a2 * w1[k] + a1 * w2[k] + a0 * w3[k];
            c3 += a2 * w0[k] + a1 * w1[k] + a0 * w2[k];
        }
        if (cs) { cs[4 * j] = c0; cs[4 * j + 1] = c1; cs[4 * j + 2] = c2; cs[4 * j + 3] = c3; }
        float u = fmaf((float)c0, 256.0f, (float)c1);
        u = fmaf(u, 256.0f, (float)c2);
        u = fmaf(u, 256.0f, (float)c3);
        y[j] = fmaf(u * sa, ai8_pow2(L->ew[j] - 18), L->bias[j]);
    }
}

/* LayerNorm in the accumulator-layout order; returns the row exponent of the output */
static int ai8_layernorm(int n, const float *x, const float *g, const float *b, float gmax, float bmax, float *y) {
    float mean, var, m = 0.0f;
    float d[ACT_H];
    if (n == ACT_H) {
        float total = 0.0f, qt = 0.0f;
        for (int blk = 0; blk < 8; blk++) {
            float s = 0.0f;
            for (int r = 0; r < 16; r++) s = s + x[ai8_feature(blk, r)];
            total = total + s;
        }
        mean = total * (1.0f / 128.0f);
        for (int j = 0; j < n; j++) d[j] = x[j] - mean;
        for (int blk = 0; blk < 8; blk++) {
            float q = 0.0f;
            for (int r = 0; r < 16; r++) { const float v = d[ai8_feature(blk, r)]; q = fmaf(v, v, q); }
            qt = qt + q;
        }
        var = qt * (1.0f / 128.0f);
    } else {
        float total = 0.0f, qt = 0.0f;
        for (int j = 0; j < n; j++) total = total + x[j];
        mean = total * (1.0f / (float)n);
        for (int j = 0; j < n; j++) d[j] = x[j] - mean;
        for (int j = 0; j < n; j++) qt = fmaf(d[j], d[j], qt);
        var = qt * (1.0f / (float)n);
    }
    for (int j = 0; j < n; j++) { const float a = fabsf(d[j]); m = a > m ? a : m; }
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int j = 0; j < n; j++) y[j] = fmaf(d[j] * rstd, g[j], b[j]);
    return ai8_exponent(fmaf(m * rstd, gmax, bmax) * 1.000001f);
}

static float ai8_absmax(int n, const float *v) {
    float m = 0.0f;
    for (int j = 0; j < n; j++) { const float a = fabsf(v[j]); m = a > m ? a : m; }
    return m;
}

/* one network: the six quantised layers and the LayerNorm bounds, built once per call */
typedef struct { ai8_layer l1, l2, gi, gh, a1, a2; float gmax[6], bmax[6]; int nobs; } ai8_net;

static int ai8_net_init(ai8_net *N, const float *w, int nobs) {
    int bad = 0;
    N->nobs = nobs;
    bad |= ai8_layer_init(&N->l1, nobs, ACT_H, ACT_H, w + ACT_L1_W, w + ACT_L1_B);
    bad |= ai8_layer_init(&N->l2, ACT_H, ACT_H, ACT_H, w + ACT_L2_W, w + ACT_L2_B);
    bad |= ai8_layer_init(&N->gi, ACT_H, 3 * ACT_H, 3 * ACT_H, w + ACT_GI_W, w + ACT_GI_B);
    bad |= ai8_layer_init(&N->gh, ACT_H, 3 * ACT_H, 3 * ACT_H, w + ACT_GH_W, w + ACT_GH_B);
    bad |= ai8_layer_init(&N->a1, ACT_H, ACT_H, ACT_H, w + ACT_A1_W, w + ACT_A1_B);
    bad |= ai8_layer_init(&N->a2, ACT_H, ACT_H, ACT_H, w + ACT_A2_W, w + ACT_A2_B);
    const int ln_g[6] = {ACT_LN0_G, ACT_LN1_G, ACT_LN2_G, ACT_LN3_G, ACT_LN4_G, ACT_LN5_G}, ln_b[6] = {ACT_LN0_B, ACT_LN1_B, ACT_LN2_B, ACT_LN3_B, ACT_LN4_B, ACT_LN5_B};
    for (int k = 0; k < 6; k++) {
        N->gmax[k] = ai8_absmax(k == 0 ? nobs : ACT_H, w + ln_g[k]);
        N->bmax[k] = ai8_absmax(k == 0 ? nobs : ACT_H, w + ln_b[k]);
    }
    return bad;
}

static void ai8_net_free(ai8_net *N) {
    ai8_layer_free(&N->l1); ai8_layer_free(&N->l2); ai8_layer_free(&N->gi); ai8_layer_free(&N->gh); ai8_layer_free(&N->a1); ai8_layer_free(&N->a2);
}

/* one row up to the output layer: m[0..3] = the head's Linear (before any tanh), h_out = the new recurrent state */
static void ai8_row(const ai8_net *N, const float *w, const float *obs, const float *h_in, float mask, float *h_out, float *m) {
    float a[ACT_H], b[ACT_H], hm[ACT_H], vi[3 * ACT_H], vh[3 * ACT_H];
    int8_t x0[ACT_H], x1[ACT_H], x2[ACT_H];
    int ex = ai8_layernorm(N->nobs, obs, w + ACT_LN0_G, w + ACT_LN0_B, N->gmax[0], N->bmax[0], b);               /* base.feature_norm */
    for (int j = 0; j < ACT_H; j++) hm[j] = h_in[j] * mask;                                                     /* gru.py:26 */
    /* non-finite rows: the observation's LayerNorm bound is an infinity or a NaN (an infinite or NaN observation, or finite ones whose sum
     * overflows) or 2^105 and more, or the masked recurrent state holds such a value (NaN * 0 is NaN) -> every output of the row is NaN, as in the
     * reference (torch propagates NaN); neither the sign nor the payload of a NaN input reaches an integer limb */
    int bad = ex >= AI8_EX_RANGE;
    for (int j = 0; j < ACT_H; j++) bad |= ai8_nonfinite(hm[j]);
    if (bad) {
        for (int j = 0; j < ACT_H; j++) h_out[j] = ai8_float(0x7FC00000u);
        for (int o = 0; o < 4; o++) m[o] = ai8_float(0x7FC00000u);
        return;
    }
    ai8_quantise(N->nobs, b, ex, x0, x1, x2);
    ai8_dense(&N->l1, x0, x1, x2, ex, a, 0);                                                                      /* base.mlp.fc.0-2 */
    act_relu(ACT_H, a);
    ex = ai8_layernorm(ACT_H, a, w + ACT_LN1_G, w + ACT_LN1_B, N->gmax[1], N->bmax[1], b);
    ai8_quantise(ACT_H, b, ex, x0, x1, x2);
    ai8_dense(&N->l2, x0, x1, x2, ex, a, 0);                                                                      /* base.mlp.fc.3-5 */
    act_relu(ACT_H, a);
    ex = ai8_layernorm(ACT_H, a, w + ACT_LN2_G, w + ACT_LN2_B, N->gmax[2], N->bmax[2], b);
    ai8_quantise(ACT_H, b, ex, x0, x1, x2);
    ai8_dense(&N->gi, x0, x1, x2, ex, vi, 0);
    const int eh = ai8_exponent(ai8_absmax(ACT_H, hm));
    ai8_quantise(ACT_H, hm, eh, x0, x1, x2);
    ai8_dense(&N->gh, x0, x1, x2, eh, vh, 0);
    for (int j = 0; j < ACT_H; j++) {
        const float r = act_sigmoid(vi[j] + vh[j]);
        const float z = act_sigmoid(vi[ACT_H + j] + vh[ACT_H + j]);
        const float nn = act_tanh(vi[2 * ACT_H + j] + r * vh[2 * ACT_H + j]);
        a[j] = (hm[j] - nn) * z + nn;
        h_out[j] = a[j];
    }
    ex = ai8_layernorm(ACT_H, a, w + ACT_LN3_G, w + ACT_LN3_B, N->gmax[3], N->bmax[3], b);                        /* rnn.norm */
    ai8_quantise(ACT_H, b, ex, x0, x1, x2);
    ai8_dense(&N->a1, x0, x1, x2, ex, a, 0);                                                                      /* act.mlp.fc.0-2 */
    act_relu(ACT_H, a);
    ex = ai8_layernorm(ACT_H, a, w + ACT_LN4_G, w + ACT_LN4_B, N->gmax[4], N->bmax[4], b);
    ai8_quantise(ACT_H, b, ex, x0, x1, x2);
    ai8_dense(&N->a2, x0, x1, x2, ex, a, 0);                                                                      /* act.mlp.fc.3-5 */
    act_relu(ACT_H, a);
    (void)ai8_layernorm(ACT_H, a, w + ACT_LN5_G, w + ACT_LN5_B, N->gmax[5], N->bmax[5], b);
    for (int o = 0; o < 4; o++) {                                                                              /* mu_net's Linear (critic: value_out in column 0) */
        float tot = w[ACT_HD_B + o];
        for (int blk = 0; blk < 8; blk++) {
            float p = 0.0f;
            for (int r = 0; r < 16; r++) { const int f = ai8_feature(blk, r); p = fmaf(w[ACT_HD_W + f * 4 + o], b[f], p); }
            tot = tot + p;
        }
        m[o] = tot;
    }
}

int f16o_actor_i8_forward(const float *w, int64_t n, const float *obs, const float *h_in, const float *mask, float *act, float *h_out) {
    ai8_net N;
    const int bad = ai8_net_init(&N, w, ACT_OBS);
    if (!bad) {
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < n; i++) {
            float m[4];
            ai8_row(&N, w, obs + ACT_OBS * i, h_in + ACT_H * i, mask[i], h_out + ACT_H * i, m);
            for (int o = 0; o < 4; o++) act[4 * i + o] = m[o] != m[o] ? m[o] : act_tanh(m[o]);                  /* mu_net: Linear + Tanh (a non-finite row: NaN) */
        }
    }
    ai8_net_free(&N);
    return bad;
}

/* f16o_policy_act (f16_actor.inc) with both networks in the block-fixed-point numerics: the same act layer / value head behind ai8_row */
int f16o_policy_act_i8(const float *wa, const float *wc, const float *std, const float *log_std, int64_t n, int obs_dim, int act_dim, int flags,
                       const float *obs, const float *ha_in, const float *hc_in, const float *mask, const float *noise, float *values,
                       float *actions, float *log_probs, float *ha_out, float *hc_out) {
    ai8_net A, Cn;
    int bad = 0;
    memset(&A, 0, sizeof A);
    memset(&Cn, 0, sizeof Cn);
    if (flags & 1) bad |= ai8_net_init(&A, wa, obs_dim);
    if (flags & 2) bad |= ai8_net_init(&Cn, wc, obs_dim);
    if (!bad) {
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < n; i++) {
            float m[4];
            if (flags & 1) {
                ai8_row(&A, wa, obs + obs_dim * i, ha_in + ACT_H * i, mask[i], ha_out + ACT_H * i, m);
                pol_sample(m, std, log_std, act_dim, flags & 4, noise ? noise + act_dim * i : 0, actions + act_dim * i, log_probs + i);
            }
            if (flags & 2) {
                ai8_row(&Cn, wc, obs + obs_dim * i, hc_in + ACT_H * i, mask[i], hc_out + ACT_H * i, m);
                values[i] = m[0];
            }
        }
    }
    if (flags & 1) ai8_net_free(&A);
    if (flags & 2) ai8_net_free(&Cn);
    return bad;
}

/* the quantised weights of one layer as this file computes them (tests compare the product's packer, neuralplane_amd/actor.py, with it):
 * layer 0 L1, 1 L2, 2 GI, 3 GH, 4 A1, 5 A2; wq[n_out][n_in] int32, ew[n_out] */
int f16o_actor_i8_weights(const float *w, int layer, int32_t *wq, int32_t *ew) {
    static const int off_w[6] = {ACT_L1_W, ACT_L2_W, ACT_GI_W, ACT_GH_W, ACT_A1_W, ACT_A2_W}, off_b[6] = {ACT_L1_B, ACT_L2_B, ACT_GI_B, ACT_GH_B, ACT_A1_B, ACT_A2_B};
    static const int n_in[6] = {ACT_OBS, ACT_H, ACT_H, ACT_H, ACT_H, ACT_H}, n_out[6] = {ACT_H, ACT_H, 3 * ACT_H, 3 * ACT_H, ACT_H, ACT_H};
    if (layer < 0 || layer > 5) return 1;
    ai8_layer L;
    if (ai8_layer_init(&L, n_in[layer], n_out[layer], n_out[layer], w + off_w[layer], w + off_b[layer])) return 1;
    for (int j = 0; j < L.n_out; j++) {
        ew[j] = L.ew[j];
        for (int k = 0; k < L.n_in; k++) {
            const size_t i = (size_t)j * L.n_in + k;
            wq[i] = ((L.limb[3][i] * 256 + L.limb[2][i]) * 256 + L.limb[1][i]) * 256 + L.limb[0][i];
        }
    }
    ai8_layer_free(&L);
    return 0;
}

/* ---- the pieces above one at a time, over arrays (tests hold each to fp64 truth; every export calls the static function the rows above use) ---- */
static int ai8_which_layer(int layer, int *n_in, int *n_out, int *off_w, int *off_b) {
    static const int ow[6] = {ACT_L1_W, ACT_L2_W, ACT_GI_W, ACT_GH_W, ACT_A1_W, ACT_A2_W}, ob[6] = {ACT_L1_B, ACT_L2_B, ACT_GI_B, ACT_GH_B, ACT_A1_B, ACT_A2_B};
    if (layer < 0 || layer > 5) return 1;
    *n_in = layer == 0 ? ACT_OBS : ACT_H;
    *n_out = layer == 2 || layer == 3 ? 3 * ACT_H : ACT_H;
    *off_w = ow[layer]; *off_b = ob[layer];
    return 0;
}

/* the quantiser: x[n_rows][n] (n <= 128) with the row exponents ex -> q[n_rows][n] (the integer before limb splitting), limbs[n_rows][3][n],
 * qsum[n_rows][n] (the magic-number sum whose low bits q is; may be 0) */
int f16o_actor_i8_quantise(int64_t n_rows, int n, const float *x, const int32_t *ex, int32_t *q, int8_t *limbs, float *qsum) {
    if (n < 1 || n > ACT_H) return 1;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; i++) {
        int8_t *l = limbs + 3 * n * i;
        ai8_quantise(n, x + n * i, ex[i], l, l + n, l + 2 * n);
        for (int k = 0; k < n; k++) {
            q[n * i + k] = ai8_q(x[n * i + k], ex[i]);
            if (qsum) qsum[n * i + k] = ai8_qsum(x[n * i + k], ex[i]);
        }
    }
    return 0;
}

/* LayerNorm `which` (0: the observation's, 22 wide; 1..5: 128 wide) of the packed network w: x[n_rows][n] -> y[n_rows][n], ex[n_rows] */
int f16o_actor_i8_layernorm(const float *w, int which, int64_t n_rows, const float *x, float *y, int32_t *ex) {
    static const int ln_g[6] = {ACT_LN0_G, ACT_LN1_G, ACT_LN2_G, ACT_LN3_G, ACT_LN4_G, ACT_LN5_G}, ln_b[6] = {ACT_LN0_B, ACT_LN1_B, ACT_LN2_B, ACT_LN3_B, ACT_LN4_B, ACT_LN5_B};
    if (which < 0 || which > 5) return 1;
    const int n = which == 0 ? ACT_OBS : ACT_H;
    const float gmax = ai8_absmax(n, w + ln_g[which]), bmax = ai8_absmax(n, w + ln_b[which]);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; i++) ex[i] = ai8_layernorm(n, x + n * i, w + ln_g[which], w + ln_b[which], gmax, bmax, y + n * i);
    return 0;
}

/* the same LayerNorm in the FIRST spec's summation order (f16_actor.inc::act_layernorm): the yardstick of the one above */
int f16o_actor_layernorm(const float *w, int which, int64_t n_rows, const float *x, float *y) {
    static const int ln_g[6] = {ACT_LN0_G, ACT_LN1_G, ACT_LN2_G, ACT_LN3_G, ACT_LN4_G, ACT_LN5_G}, ln_b[6] = {ACT_LN0_B, ACT_LN1_B, ACT_LN2_B, ACT_LN3_B, ACT_LN4_B, ACT_LN5_B};
    if (which < 0 || which > 5) return 1;
    const int n = which == 0 ? ACT_OBS : ACT_H;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; i++) act_layernorm(n, x + n * i, w + ln_g[which], w + ln_b[which], y + n * i);
    return 0;
}

/* quantised Linear `layer` (0 L1 .. 5 A2): x[n_rows][n_in] with the row exponents ex -> y[n_rows][n_out] and the class sums c[n_rows][n_out][4] */
int f16o_actor_i8_dense(const float *w, int layer, int64_t n_rows, const float *x, const int32_t *ex, float *y, int32_t *c) {
    int n_in, n_out, off_w, off_b;
    if (ai8_which_layer(layer, &n_in, &n_out, &off_w, &off_b)) return 1;
    ai8_layer L;
    if (ai8_layer_init(&L, n_in, n_out, n_out, w + off_w, w + off_b)) return 1;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n_rows; i++) {
        int8_t x0[ACT_H], x1[ACT_H], x2[ACT_H];
        ai8_quantise(n_in, x + (int64_t)n_in * i, ex[i], x0, x1, x2);
        ai8_dense(&L, x0, x1, x2, ex[i], y + (int64_t)n_out * i, c + 4 * (int64_t)n_out * i);
    }
    ai8_layer_free(&L);
    return 0;
}
