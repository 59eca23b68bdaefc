// np_model_jets.h — the device code the model-side derivative kernels share: F16Dynamics.nlplant on value + tangent pairs ("jets").
//   - phase 1: the 42 live nets with their 1-3 input derivatives (forward mode: a tangent chain beside the value chain), the weights read
//     from the single-set blob in LDS (LdsRec), split over eight waves by PLAN8_LIN: 110 columns per row, plus the 12 shared scalars of the
//     state (lin_phase1);
//   - phase 2: the coefficient build-up and the equations of motion on Jet<N> (nlplant_jets), the value halves the spec's operations one for one.
// Used by np_model_linearize.hip (which stores the tangents: A and B) and np_model_rollout_vjp.hip (which contracts them with an adjoint).
#pragma once
#include "np_model_linearize.h"

#include "np_f16_device.h"
#include "np_f16_kargs.h"

namespace npf16 {

// ---- the 110 columns: per output slot (class order, np_nets.h) the value, then one derivative per input of the net's class ----------------
constexpr int class_of_slot(int slot) {
    for (int cl = 0; cl < NUM_CLASSES; cl++)
        if (slot < class_slot(cl) + CLASSES[cl].count) return cl;
    return NUM_CLASSES - 1;
}
constexpr int lin_col(int slot) {
    int c = 0;
    for (int s = 0; s < slot; s++) c += 1 + CLASSES[class_of_slot(s)].n_in;
    return c;
}
constexpr int LIN_COLS = lin_col(NUM_LIVE_NETS);
static_assert(LIN_COLS == 110, "42 values + 68 input derivatives");
static_assert(KBLOB_FLOATS % 4 == 0 && KBLOB_HEADER % 4 == 0 && ASM_GROUP % 4 == 0, "the blob and every record in it are whole 16-byte vectors");
constexpr int LIN_LDS_FLOATS = KBLOB_FLOATS + (LIN_COLS + NUM_SHARED_SCALARS) * LIN_TILE;
static_assert(LIN_LDS_FLOATS * sizeof(float) <= 160 * 1024, "blob + columns + shared scalars fit a CU's LDS");

// ---- phase 1's plan: which wave evaluates which nets; cost of a net = its parameters x (1 + inputs) ------------------------------------
constexpr SplitPlan PLAN8_LIN = {{{{CL_F, 0, 2}, NO_ITEM, NO_ITEM, NO_ITEM},
                                  {{CL_F, 2, 1}, {CL_C, 0, 2}, NO_ITEM, NO_ITEM},
                                  {{CL_C, 2, 3}, {CL_D_RUD, 0, 1}, NO_ITEM, NO_ITEM},
                                  {{CL_E_LEF, 0, 4}, {CL_ETA, 0, 1}, NO_ITEM, NO_ITEM},
                                  {{CL_E_RUD, 0, 4}, {CL_DLEF, 6, 1}, NO_ITEM, NO_ITEM},
                                  {{CL_YA20, 0, 1}, {CL_D_RUD, 1, 1}, {CL_D_LEF, 0, 2}, {CL_YPLEF, 0, 1}},
                                  {{CL_DAMP, 0, 9}, NO_ITEM, NO_ITEM, NO_ITEM},
                                  {{CL_DAMP, 9, 3}, {CL_DLEF, 0, 6}, NO_ITEM, NO_ITEM}}};
static_assert(plan_covers(PLAN8_LIN, AB_ALL, 5, 1), "the linearisation plan must cover every live net exactly once");
constexpr int lin_wave_cost(int w) {
    int c = 0;
    for (int k = 0; k < SPLIT_MAX; k++)
        if (PLAN8_LIN.it[w][k].cnt > 0) c += PLAN8_LIN.it[w][k].cnt * class_params(CLASSES[PLAN8_LIN.it[w][k].cl]) * (1 + CLASSES[PLAN8_LIN.it[w][k].cl].n_in);
    return c;
}
constexpr bool lin_plan_balanced() {  // no wave more than 6 % above the mean
    int tot = 0;
    for (int w = 0; w < LIN_WAVES; w++) tot += lin_wave_cost(w);
    for (int w = 0; w < LIN_WAVES; w++)
        if (lin_wave_cost(w) * LIN_WAVES * 100 > tot * 106) return false;
    return true;
}
static_assert(lin_plan_balanced(), "PLAN8_LIN is balanced by parameters x (1 + inputs)");

// ---- a net's record in LDS, read without state: the position of a weight in its record follows from the layer's place in the record and
// the loop indices, compile-time constants after unrolling, so a row of weights is the few 128-bit reads (ds_read_b128 at (wave-uniform
// record base) + constant) that cover it, and a weight is an element of one of them.
// The order of reads and FMAs is fixed by two chain values (opaque zeros added to the record's offset).  Row k of a layer reads through
// chain k % 2, and when its FMAs are written down the row's accumulators become inputs of an opaque statement on that chain: the FMAs of
// row k come before that statement, the reads of row k + 2 after it.  So at most two rows of weights are in registers, and the reads of
// row k + 1 are in flight behind the FMAs of row k.  Left alone, instruction selection emits a net's reads first and its FMAs last — every
// weight of the net live in between, in scratch.  The chains run on from net to net.
struct LdsRec {
    const f32x4 *blob4;  // the blob in LDS
    int rec;             // the record's position in it, in vectors (wave-uniform)
    int chain[2];
    // floats [p0, p0 + LEN) of the record as whole vectors; the opaque statement keeps each a 128-bit read (left visible, the compiler
    // narrows the read of a vector whose elements are used one by one into four 32-bit reads)
    template <int LEN>
    struct Row {
        static constexpr int NV = LEN / 4 + 2;
        f32x4 v[NV];
        int first;
        __device__ __forceinline__ float operator[](int p) const { return v[(p >> 2) - first][p & 3]; }
    };
    template <int LEN>
    __device__ __forceinline__ Row<LEN> row(int p0, int which = 0) const {
        Row<LEN> r;
        r.first = p0 >> 2;
#pragma unroll
        for (int i = 0; i < Row<LEN>::NV; i++)
            if (r.first + i <= ((p0 + LEN - 1) >> 2)) {
                r.v[i] = blob4[rec + chain[which] + r.first + i];
                asm("" : "+v"(r.v[i]));
            }
        return r;
    }
    template <int NT, int OUT>
    __device__ __forceinline__ void tie(int which, const float (&y)[OUT], const float (&ty)[NT][OUT]) {
        static_assert(OUT % 5 == 0, "layer widths are multiples of five");
#pragma unroll
        for (int j = 0; j < OUT; j += 5) {
            asm volatile("" : "+v"(chain[which]) : "v"(y[j]), "v"(y[j + 1]), "v"(y[j + 2]), "v"(y[j + 3]), "v"(y[j + 4]));
#pragma unroll
            for (int i = 0; i < NT; i++)
                asm volatile("" : "+v"(chain[which]) : "v"(ty[i][j]), "v"(ty[i][j + 1]), "v"(ty[i][j + 2]), "v"(ty[i][j + 3]), "v"(ty[i][j + 4]));
        }
    }
};

// the clamp of the spec on an activation carried / 2^ACT_SHIFT, and its derivative: 1 strictly inside (0, 1), 0 elsewhere (exactly 0 gives 0)
template <int NT, int OUT>
__device__ __forceinline__ void clamp_jet(float (&y)[OUT], float (&ty)[NT][OUT]) {
#pragma unroll
    for (int j = 0; j < OUT; j++) {
        const bool inside = y[j] > 0.0f && y[j] < 1.0f;
        y[j] = y[j] > 0.0f ? y[j] : 0.0f;
        y[j] = y[j] > 1.0f ? 1.0f : y[j];
#pragma unroll
        for (int i = 0; i < NT; i++) ty[i][j] = inside ? ty[i][j] : 0.0f;
    }
}

// A hidden layer at float BASE of the record: bias[OUT] then W^T[IN][OUT], rows padded to an even length (np_nets.h::asm_record_len)
constexpr int dense_len(int in, int out) { return (1 + in) * pad2(out); }

// first hidden layer: the tangent of pre-activation j in the direction of input i is the weight itself
template <int BASE, int IN, int OUT>
__device__ __forceinline__ void dense_jet_first(LdsRec &ws, const float (&x)[IN], float (&y)[OUT], float (&ty)[IN][OUT]) {
    const auto bias = ws.template row<OUT>(BASE);
#pragma unroll
    for (int j = 0; j < OUT; j++) y[j] = bias[BASE + j];
#pragma unroll
    for (int k = 0; k < IN; k++) {
        const int p0 = BASE + (1 + k) * pad2(OUT);
        const auto wk = ws.template row<OUT>(p0, k & 1);
#pragma unroll
        for (int j = 0; j < OUT; j++) {
            const float w = wk[p0 + j];
            y[j] = fmaf(w, x[k], y[j]);
            ty[k][j] = w;
        }
    }
    ws.template tie<IN, OUT>(0, y, ty);
    clamp_jet<IN, OUT>(y, ty);
}

// a later hidden layer: value chain bias first, tangent chains without a bias, all in the order the weights come (k ascending)
template <int BASE, int NT, int IN, int OUT>
__device__ __forceinline__ void dense_jet(LdsRec &ws, const float (&x)[IN], const float (&tx)[NT][IN], float (&y)[OUT], float (&ty)[NT][OUT]) {
    const auto bias = ws.template row<OUT>(BASE);
#pragma unroll
    for (int j = 0; j < OUT; j++) y[j] = bias[BASE + j];
#pragma unroll
    for (int k = 0; k < IN; k++) {
        const int p0 = BASE + (1 + k) * pad2(OUT);
        const auto wk = ws.template row<OUT>(p0, k & 1);
#pragma unroll
        for (int j = 0; j < OUT; j++) {
            const float w = wk[p0 + j];
            y[j] = fmaf(w, x[k], y[j]);
#pragma unroll
            for (int i = 0; i < NT; i++) ty[i][j] = k == 0 ? w * tx[i][0] : fmaf(w, tx[i][k], ty[i][j]);
        }
        ws.template tie<NT, OUT>(k & 1, y, ty);
    }
    clamp_jet<NT, OUT>(y, ty);
}

// output layer in -> 1 at float BASE: (bias, 0), W[0][0..IN) padded to even.  Two interleaved partial chains from (bias, 0), even inputs to
// the first, odd to the second, an odd last input to the first; y = lo + hi.  The tangents take the same two chains from (0, 0).
template <int BASE, int NT, int IN>
__device__ __forceinline__ void out_jet(LdsRec &ws, const float (&x)[IN], const float (&tx)[NT][IN], float &y, float (&ty)[NT], float &out_std, float &out_mean) {
    const auto r = ws.template row<4 + pad2(IN)>(BASE);  // the layer, then out_std and out_mean
    out_std = r[BASE + 2 + pad2(IN)];
    out_mean = r[BASE + 3 + pad2(IN)];
    float lo = r[BASE], hi = r[BASE + 1];
    float tlo[NT], thi[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) tlo[i] = thi[i] = 0.0f;
#pragma unroll
    for (int k = 0; k + 1 < IN; k += 2) {
        const float w0 = r[BASE + 2 + k], w1 = r[BASE + 3 + k];
        lo = fmaf(w0, x[k], lo);
        hi = fmaf(w1, x[k + 1], hi);
#pragma unroll
        for (int i = 0; i < NT; i++) {
            tlo[i] = fmaf(w0, tx[i][k], tlo[i]);
            thi[i] = fmaf(w1, tx[i][k + 1], thi[i]);
        }
    }
    if (IN & 1) {
        const float w0 = r[BASE + 2 + IN - 1];
        lo = fmaf(w0, x[IN - 1], lo);
#pragma unroll
        for (int i = 0; i < NT; i++) tlo[i] = fmaf(w0, tx[i][IN - 1], tlo[i]);
    }
    y = lo + hi;
#pragma unroll
    for (int i = 0; i < NT; i++) ty[i] = tlo[i] + thi[i];
}

// one net: y = unnormalised output, dy[i] = dy / d(normalised input i)
template <int IN, int H1, int H2, int H3>
__device__ __forceinline__ void net_jet(LdsRec &ws, const float (&x)[IN], float &y, float (&dy)[IN]) {
    constexpr int B2 = dense_len(IN, H1), B3 = B2 + dense_len(H1, H2), HL = H3 > 0 ? H3 : H2;
    constexpr int BO = H3 > 0 ? B3 + dense_len(H2, H3) : B3, BS = BO + 2 + pad2(HL);
    static_assert(BS + 2 <= asm_record_len(IN, H1, H2, H3), "the layers' places add up to the record (np_nets.h::asm_record_len)");
    float h1[H1], t1[IN][H1], h2[H2], t2[IN][H2];
    dense_jet_first<0, IN, H1>(ws, x, h1, t1);
    dense_jet<B2, IN, H1, H2>(ws, h1, t1, h2, t2);
    float yn, tn[IN], out_std, out_mean;
    if constexpr (H3 > 0) {
        float h3[H3], t3[IN][H3];
        dense_jet<B3, IN, H2, H3>(ws, h2, t2, h3, t3);
        out_jet<BO, IN, H3>(ws, h3, t3, yn, tn, out_std, out_mean);
    } else {
        out_jet<BO, IN, H2>(ws, h2, t2, yn, tn, out_std, out_mean);
    }
    y = yn * out_std + out_mean;  // unnormalize: X * std + mean
#pragma unroll
    for (int i = 0; i < IN; i++) dy[i] = tn[i] * out_std;
}

// nets [FIRST, FIRST + COUNT) of class CL -> this lane's columns: value, then d/d(alpha_deg | beta_deg | el) = d/d(normalised input) x RN(1 / sigma)
template <int CL, int FIRST, int COUNT>
__device__ __forceinline__ void eval_class_jet(LdsRec &ws, const float *blob, const float (&xn)[NUM_NORM_GROUPS], float *col) {
    constexpr NetClass c = CLASSES[CL];
    static_assert(COUNT > 0 && FIRST >= 0 && FIRST + COUNT <= c.count, "class range");
    float x[c.n_in], rs[c.n_in];
#pragma unroll
    for (int k = 0; k < c.n_in; k++) {
        x[k] = xn[c.grp[k]];
        rs[k] = blob[KBLOB_NORM_STRIDE * c.grp[k] + 2];
    }
    // one net at a time: a whole net is the loop body, and interleaving two of them would double the live registers
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = 0; i < COUNT; i++) {
        float y, dy[c.n_in];
        ws.rec = (class_base(CL) + (FIRST + i) * class_stride(CL)) / 4;
        net_jet<c.n_in, c.h1, c.h2, c.h3>(ws, x, y, dy);
        float *o = col + (lin_col(class_slot(CL) + FIRST) + i * (1 + c.n_in)) * LIN_TILE;
        o[0] = y;
#pragma unroll
        for (int k = 0; k < c.n_in; k++) o[(1 + k) * LIN_TILE] = dy[k] * rs[k];
    }
}

template <int W>
__device__ __forceinline__ void eval_plan_jet(const float *blob, const float (&xn)[NUM_NORM_GROUPS], float *col) {
    LdsRec ws = {(const f32x4 *)blob, 0, {0, 0}};
#define NPF16_ITEM(K) \
    if constexpr (PLAN8_LIN.it[W][K].cnt > 0) eval_class_jet<PLAN8_LIN.it[W][K].cl, PLAN8_LIN.it[W][K].first, PLAN8_LIN.it[W][K].cnt>(ws, blob, xn, col)
    NPF16_ITEM(0);
    NPF16_ITEM(1);
    NPF16_ITEM(2);
    NPF16_ITEM(3);
#undef NPF16_ITEM
}

// ---- the same nets by value only (np_model_trim.hip's backtracking pass): the value chains above, operation for operation and in the same
// order (bias first, k ascending; the output layer's two interleaved partial chains), without the tangent chains beside them.  The reads
// and FMAs are ordered by the same two chain values.  The value of slot `slot` goes where eval_class_jet puts it, column lin_col(slot); the
// derivative columns are left as they are (nobody reads them after a value pass) ----
template <int OUT>
__device__ __forceinline__ void tie_val(LdsRec &ws, int which, const float (&y)[OUT]) {
    static_assert(OUT % 5 == 0, "layer widths are multiples of five");
#pragma unroll
    for (int j = 0; j < OUT; j += 5) asm volatile("" : "+v"(ws.chain[which]) : "v"(y[j]), "v"(y[j + 1]), "v"(y[j + 2]), "v"(y[j + 3]), "v"(y[j + 4]));
}
template <int BASE, int IN, int OUT>
__device__ __forceinline__ void dense_val(LdsRec &ws, const float (&x)[IN], float (&y)[OUT]) {
    const auto bias = ws.template row<OUT>(BASE);
#pragma unroll
    for (int j = 0; j < OUT; j++) y[j] = bias[BASE + j];
#pragma unroll
    for (int k = 0; k < IN; k++) {
        const int p0 = BASE + (1 + k) * pad2(OUT);
        const auto wk = ws.template row<OUT>(p0, k & 1);
#pragma unroll
        for (int j = 0; j < OUT; j++) y[j] = fmaf(wk[p0 + j], x[k], y[j]);
        tie_val<OUT>(ws, k & 1, y);
    }
#pragma unroll
    for (int j = 0; j < OUT; j++) {
        y[j] = y[j] > 0.0f ? y[j] : 0.0f;
        y[j] = y[j] > 1.0f ? 1.0f : y[j];
    }
}
template <int BASE, int IN>
__device__ __forceinline__ float out_val(LdsRec &ws, const float (&x)[IN]) {
    const auto r = ws.template row<4 + pad2(IN)>(BASE);  // the layer, then out_std and out_mean
    float lo = r[BASE], hi = r[BASE + 1];
#pragma unroll
    for (int k = 0; k + 1 < IN; k += 2) {
        lo = fmaf(r[BASE + 2 + k], x[k], lo);
        hi = fmaf(r[BASE + 3 + k], x[k + 1], hi);
    }
    if (IN & 1) lo = fmaf(r[BASE + 2 + IN - 1], x[IN - 1], lo);
    return (lo + hi) * r[BASE + 2 + pad2(IN)] + r[BASE + 3 + pad2(IN)];  // unnormalize: X * std + mean
}
template <int IN, int H1, int H2, int H3>
__device__ __forceinline__ float net_val(LdsRec &ws, const float (&x)[IN]) {
    constexpr int B2 = dense_len(IN, H1), B3 = B2 + dense_len(H1, H2), BO = H3 > 0 ? B3 + dense_len(H2, H3) : B3;
    float h1[H1], h2[H2];
    dense_val<0, IN, H1>(ws, x, h1);
    dense_val<B2, H1, H2>(ws, h1, h2);
    if constexpr (H3 > 0) {
        float h3[H3];
        dense_val<B3, H2, H3>(ws, h2, h3);
        return out_val<BO, H3>(ws, h3);
    } else {
        return out_val<BO, H2>(ws, h2);
    }
}
template <int CL, int FIRST, int COUNT>
__device__ __forceinline__ void eval_class_val(LdsRec &ws, const float (&xn)[NUM_NORM_GROUPS], float *col) {
    constexpr NetClass c = CLASSES[CL];
    float x[c.n_in];
#pragma unroll
    for (int k = 0; k < c.n_in; k++) x[k] = xn[c.grp[k]];
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = 0; i < COUNT; i++) {
        ws.rec = (class_base(CL) + (FIRST + i) * class_stride(CL)) / 4;
        col[(lin_col(class_slot(CL) + FIRST) + i * (1 + c.n_in)) * LIN_TILE] = net_val<c.n_in, c.h1, c.h2, c.h3>(ws, x);
    }
}
template <int W>
__device__ __forceinline__ void eval_plan_val(const float *blob, const float (&xn)[NUM_NORM_GROUPS], float *col) {
    LdsRec ws = {(const f32x4 *)blob, 0, {0, 0}};
#define NPF16_ITEM(K) \
    if constexpr (PLAN8_LIN.it[W][K].cnt > 0) eval_class_val<PLAN8_LIN.it[W][K].cl, PLAN8_LIN.it[W][K].first, PLAN8_LIN.it[W][K].cnt>(ws, xn, col)
    NPF16_ITEM(0);
    NPF16_ITEM(1);
    NPF16_ITEM(2);
    NPF16_ITEM(3);
#undef NPF16_ITEM
}

// ---- phase 2: value + N tangents.  The value halves are the spec's operations, one for one; the tangents are the chain rule ----------------
template <int N>
struct Jet {
    float v, d[N];
};
#define NPJ_EACH for (int n_ = 0; n_ < N; n_++)
template <int N>
__device__ __forceinline__ Jet<N> operator+(const Jet<N> &a, const Jet<N> &b) {
    Jet<N> r;
    r.v = a.v + b.v;
#pragma unroll
    NPJ_EACH r.d[n_] = a.d[n_] + b.d[n_];
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator+(const Jet<N> &a, float b) {
    Jet<N> r = a;
    r.v = a.v + b;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator-(const Jet<N> &a, const Jet<N> &b) {
    Jet<N> r;
    r.v = a.v - b.v;
#pragma unroll
    NPJ_EACH r.d[n_] = a.d[n_] - b.d[n_];
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(const Jet<N> &a, const Jet<N> &b) {
    Jet<N> r;
    r.v = a.v * b.v;
#pragma unroll
    NPJ_EACH r.d[n_] = fmaf(a.d[n_], b.v, a.v * b.d[n_]);
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(const Jet<N> &a, float b) {
    Jet<N> r;
    r.v = a.v * b;
#pragma unroll
    NPJ_EACH r.d[n_] = a.d[n_] * b;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(float a, const Jet<N> &b) {
    Jet<N> r;
    r.v = a * b.v;
#pragma unroll
    NPJ_EACH r.d[n_] = a * b.d[n_];
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator/(const Jet<N> &a, const Jet<N> &b) {
    Jet<N> r;
    r.v = a.v / b.v;
#pragma unroll
    NPJ_EACH r.d[n_] = (a.d[n_] - r.v * b.d[n_]) / b.v;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator/(float a, const Jet<N> &b) {
    Jet<N> r;
    r.v = a / b.v;
#pragma unroll
    NPJ_EACH r.d[n_] = -(r.v * b.d[n_]) / b.v;
    return r;
}
// division by a constant (np_divc): the tangent is scaled by the prepared reciprocal
template <int N>
__device__ __forceinline__ Jet<N> divc_jet(const Jet<N> &x, float c, float rc) {
    Jet<N> r;
    r.v = np_divc(x.v, c, rc);
#pragma unroll
    NPJ_EACH r.d[n_] = x.d[n_] * rc;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> poison_jet(bool ok, const Jet<N> &x) {
    const float qnan = __builtin_nanf("");
    Jet<N> r;
    r.v = ok ? x.v : qnan;
#pragma unroll
    NPJ_EACH r.d[n_] = ok ? x.d[n_] : qnan;
    return r;
}

// the directions of phase 2, in the order of [A | B]'s non-trivial columns
enum LinDir : int { D_ALT, D_PHI, D_THETA, D_PSI, D_VT, D_ALPHA, D_BETA, D_P, D_Q, D_R, D_T, D_EL, D_AIL, D_RUD, NUM_LIN_DIRS };

// coefficient `ID` as a jet: value and input derivatives from the lane's columns, chained to the inputs' tangents
template <int ID, int N>
__device__ __forceinline__ Jet<N> coef_jet(const float *col, const Jet<N> &a_deg, const Jet<N> &b_deg, const Jet<N> &el) {
    constexpr int slot = slot_of(ID), c0 = lin_col(slot);
    static_assert(slot >= 0, "a live net");
    constexpr NetClass c = CLASSES[class_of_slot(slot)];
    Jet<N> r;
    r.v = col[c0 * LIN_TILE];
#pragma unroll
    for (int k = 0; k < c.n_in; k++) {
        const float p = col[(c0 + 1 + k) * LIN_TILE];
        const Jet<N> &in = c.grp[k] <= G_A_RUD ? a_deg : c.grp[k] <= G_B_O ? b_deg : el;
#pragma unroll
        NPJ_EACH r.d[n_] = k == 0 ? p * in.d[n_] : fmaf(p, in.d[n_], r.d[n_]);
    }
    return r;
}

// F16Dynamics.nlplant on jets: np_f16_device.h::nlplant<FULL> operation for operation (same grouping, same order), the shared scalars of
// the state from `shr`, the coefficients from `col`; dir[n] is the direction of tangent n (or -1: all-zero seeds, nothing stored)
template <int N, class AF>  // AF: Airframe, or Airframe in the constant address space
__device__ __forceinline__ void nlplant_jets(const AF &af, const float (&s)[12], const float (&u)[4], const float *shr, const float *col,
                                             const int (&dir)[N], bool ok, Jet<N> (&xd)[12]) {
    const float r2d = (float)(180.0 / 3.141592653589793);
    auto seeded = [&dir](float v, int k, float scale = 1.0f) {
        Jet<N> r;
        r.v = v;
#pragma unroll
        NPJ_EACH r.d[n_] = dir[n_] == k ? scale : 0.0f;
        return r;
    };
    auto with_slope = [&dir](float v, int k, float slope) {  // a function of input k alone
        Jet<N> r;
        r.v = v;
#pragma unroll
        NPJ_EACH r.d[n_] = (dir[n_] == k ? 1.0f : 0.0f) * slope;
        return r;
    };
    const Jet<N> alt = seeded(s[2], D_ALT), vt0 = seeded(s[6], D_VT);
    const Jet<N> alpha = seeded(s[7] * r2d, D_ALPHA, r2d), beta = seeded(s[8] * r2d, D_BETA, r2d);  // degrees
    const Jet<N> P = seeded(s[9], D_P), Q = seeded(s[10], D_Q), R = seeded(s[11], D_R);
    const Jet<N> T = seeded(u[0], D_T), el = seeded(u[1], D_EL), ail = seeded(u[2], D_AIL), rud = seeded(u[3], D_RUD);

    const float sa_ = shr[0 * LIN_TILE], ca_ = shr[1 * LIN_TILE], sb_ = shr[2 * LIN_TILE], cb_ = shr[3 * LIN_TILE];
    const float st_ = shr[4 * LIN_TILE], ct_ = shr[5 * LIN_TILE], sphi_ = shr[6 * LIN_TILE], cphi_ = shr[7 * LIN_TILE];
    const float tt_ = shr[8 * LIN_TILE], spsi_ = shr[9 * LIN_TILE], cpsi_ = shr[10 * LIN_TILE], powv_ = shr[11 * LIN_TILE];
    const Jet<N> sa = with_slope(sa_, D_ALPHA, ca_), ca = with_slope(ca_, D_ALPHA, -sa_);
    const Jet<N> sb = with_slope(sb_, D_BETA, cb_), cb = with_slope(cb_, D_BETA, -sb_);
    const Jet<N> st = with_slope(st_, D_THETA, ct_), ct = with_slope(ct_, D_THETA, -st_), tt = with_slope(tt_, D_THETA, 1.0f + tt_ * tt_);
    const Jet<N> sphi = with_slope(sphi_, D_PHI, cphi_), cphi = with_slope(cphi_, D_PHI, -sphi_);
    const Jet<N> spsi = with_slope(spsi_, D_PSI, cpsi_), cpsi = with_slope(cpsi_, D_PSI, -spsi_);
    // d(tfac^e)/d(alt) = -e * lapse * tfac^e / tfac
    const float tfac = 1.0f - af.atm_lapse * s[2];
    const Jet<N> powv = with_slope(powv_, D_ALT, ((-(float)af.atm_exp * af.atm_lapse) * powv_) / tfac);

    const float g = af.g, mass = af.mass, B = af.B, S = af.S, cbar = af.cbar, Heng = af.Heng;
    const float Jy = af.Jy, Jxz = af.Jxz, Jz = af.Jz, Jx = af.Jx;
    const float xc = af.xc, cbar_over_B = af.cbar_over_B, c1 = af.c1, c2 = af.c2, c3 = af.c3, c4 = af.c4, denom = af.denom;

    // vt = (vt <= 0.01) * 0.01 + (vt > 0.01) * vt (:104), differentiated as written: a product with a mask
    const float m_lo = vt0.v <= 0.01f ? 1.0f : 0.0f, m_hi = vt0.v > 0.01f ? 1.0f : 0.0f;
    Jet<N> vt;
    vt.v = m_lo * 0.01f + m_hi * vt0.v;
#pragma unroll
    NPJ_EACH vt.d[n_] = m_hi * vt0.d[n_];

    const Jet<N> dail = divc_jet(ail, af.ail_ref, af.r_ail_ref), drud = divc_jet(rud, af.rud_ref, af.r_rud_ref);
    const Jet<N> rho = af.rho0 * powv;
    const Jet<N> qbar = (0.5f * rho) * (vt * vt);
    const Jet<N> U = (vt * ca) * cb, V = vt * sb, W = (vt * sa) * cb;

    xd[0] = (U * (ct * cpsi) + V * ((sphi * cpsi) * st - cphi * spsi)) + W * ((cphi * st) * cpsi + sphi * spsi);
    xd[1] = (U * (ct * spsi) + V * ((sphi * spsi) * st + cphi * cpsi)) + W * ((cphi * st) * spsi - sphi * cpsi);
    xd[2] = (U * st - V * (sphi * ct)) - W * (cphi * ct);
    xd[3] = P + tt * (Q * sphi + R * cphi);
    xd[4] = Q * cphi - R * sphi;
    xd[5] = (Q * sphi + R * cphi) / ct;

    const Jet<N> inv2vt = 1.0f / (2.0f * vt);
    const Jet<N> c2v = inv2vt * cbar;
    const Jet<N> b2v = inv2vt * B;

#define NPF16_NET(id) coef_jet<id, N>(col, alpha, beta, el)
#define NPF16_POISON(v) poison_jet(ok, (v))
    // --- X / Z force ---------------------------------------------------------------------
    const Jet<N> dCx_lef = NPF16_NET(N_dCx_lef);
    const Jet<N> dXdQ = c2v * (NPF16_NET(N_Cxq) + NPF16_NET(N_dCxq_lef));
    const Jet<N> Cx_tot = NPF16_POISON((NPF16_NET(N_Cx) + dCx_lef) + dXdQ * Q);
    const Jet<N> dCz_lef = NPF16_NET(N_dCz_lef);
    const Jet<N> dZdQ = c2v * (NPF16_NET(N_Czq) + dCz_lef);  // reference uses delta_Cz_lef here (:199)
    const Jet<N> Cz_tot = NPF16_POISON((NPF16_NET(N_Cz) + dCz_lef) + dZdQ * Q);
    // --- Y force ---------------------------------------------------------------------------
    const Jet<N> dYdail = NPF16_NET(N_dCy_a20) + NPF16_NET(N_dCy_a20_lef);
    const Jet<N> dYdR = b2v * (NPF16_NET(N_Cyr) + NPF16_NET(N_dCyr_lef));
    const Jet<N> dYdP = b2v * (NPF16_NET(N_Cyp) + NPF16_NET(N_dCyp_lef));
    const Jet<N> Cy_tot =
        NPF16_POISON(((((NPF16_NET(N_Cy) + NPF16_NET(N_dCy_lef)) + dYdail * dail) + NPF16_NET(N_dCy_r30) * drud) + dYdR * R) + dYdP * P);

    const float r_mass = af.r_mass;
    const Jet<N> Udot = (((R * V - Q * W) - g * st) + divc_jet((qbar * S) * Cx_tot, mass, r_mass)) + divc_jet(T, mass, r_mass);
    const Jet<N> Vdot = ((P * W - R * U) + (g * ct) * sphi) + divc_jet((qbar * S) * Cy_tot, mass, r_mass);
    const Jet<N> Wdot = ((Q * U - P * V) + (g * ct) * cphi) + divc_jet((qbar * S) * Cz_tot, mass, r_mass);
    xd[6] = ((U * Udot + V * Vdot) + W * Wdot) / vt;
    xd[7] = (U * Wdot - W * Udot) / (U * U + W * W);
    xd[8] = (Vdot * vt - V * xd[6]) / ((vt * vt) * cb);

    // --- pitching moment ----------------------------------------------------------------
    const Jet<N> dMdQ = c2v * (NPF16_NET(N_Cmq) + NPF16_NET(N_dCmq_lef));
    const Jet<N> Cm_tot =
        NPF16_POISON(((((NPF16_NET(N_Cm) * NPF16_NET(N_eta_el) + Cz_tot * xc) + NPF16_NET(N_dCm_lef)) + dMdQ * Q) + NPF16_NET(N_dCm)) + 0.0f);
    // --- yawing moment ------------------------------------------------------------------
    const Jet<N> dNdail = NPF16_NET(N_dCn_a20) + NPF16_NET(N_dCn_a20_lef);
    const Jet<N> dNdR = b2v * (NPF16_NET(N_Cnr) + NPF16_NET(N_dCnr_lef));
    const Jet<N> dNdP = b2v * (NPF16_NET(N_Cnp) + NPF16_NET(N_dCnp_lef));
    const Jet<N> Cn_tot = NPF16_POISON(((((((NPF16_NET(N_Cn) + NPF16_NET(N_dCn_lef)) - (Cy_tot * xc) * cbar_over_B) + dNdail * dail) +
                                         NPF16_NET(N_dCn_r30) * drud) + dNdR * R) + dNdP * P) + NPF16_NET(N_dCnbeta) * beta);
    // --- rolling moment -----------------------------------------------------------------
    const Jet<N> dLdail = NPF16_NET(N_dCl_a20) + NPF16_NET(N_dCl_a20_lef);
    const Jet<N> dLdR = b2v * (NPF16_NET(N_Clr) + NPF16_NET(N_dClr_lef));
    const Jet<N> dLdP = b2v * (NPF16_NET(N_Clp) + NPF16_NET(N_dClp_lef));
    const Jet<N> Cl_tot = NPF16_POISON((((((NPF16_NET(N_Cl) + NPF16_NET(N_dCl_lef)) + dLdail * dail) + NPF16_NET(N_dCl_r30) * drud) +
                                        dLdR * R) + dLdP * P) + NPF16_NET(N_dClbeta) * beta);
#undef NPF16_NET
#undef NPF16_POISON

    const Jet<N> L_tot = ((Cl_tot * qbar) * S) * B;
    const Jet<N> M_tot = ((Cm_tot * qbar) * S) * cbar;
    const Jet<N> N_tot = ((Cn_tot * qbar) * S) * B;
    xd[9] = divc_jet((((Jz * L_tot + Jxz * N_tot) - (c1 * Q) * R) + (c2 * P) * Q) + (Jxz * Q) * Heng, denom, af.r_denom);
    xd[10] = divc_jet(((M_tot + (c3 * P) * R) - Jxz * (P * P - R * R)) - R * Heng, Jy, af.r_Jy);
    xd[11] = divc_jet((((Jx * N_tot + Jxz * L_tot) + (c4 * P) * Q) - (c2 * Q) * R) + (Jx * Q) * Heng, denom, af.r_denom);
}
#undef NPJ_EACH

// ---- phase 1 of a tile: wave `pw` evaluates its slice of PLAN8_LIN into the lane's columns; three of the lighter waves also compute the
// serial fp64 chains of the state (state(k) = the row's state k) into the tile's shared scalars.  f16_linearize_kernel spells the same chain
// out in place: called from here its instruction order and register allocation change (217 VGPRs against 220), and that kernel is kept as
// it was measured ----
template <class AF, class State>
__device__ __forceinline__ void lin_phase1(int pw, const AF &af, const float *blob, const float (&xn)[NUM_NORM_GROUPS], float *col, float *shr, State state) {
    if (pw == 0) {  // the lightest slice of the plan also takes theta, phi and the atmosphere power
        float a_, b_, c_;
        np_sincostan(state(4), a_, b_, c_);
        shr[4 * LIN_TILE] = a_;
        shr[5 * LIN_TILE] = b_;
        shr[8 * LIN_TILE] = c_;
        np_sincos(state(3), a_, b_);
        shr[6 * LIN_TILE] = a_;
        shr[7 * LIN_TILE] = b_;
        shr[11 * LIN_TILE] = atmos_pow(af, state(2));
        eval_plan_jet<0>(blob, xn, col);
    } else if (pw == 1) {
        eval_plan_jet<1>(blob, xn, col);
    } else if (pw == 2) {
        float a_, b_;
        np_sincos(state(5), a_, b_);
        shr[9 * LIN_TILE] = a_;
        shr[10 * LIN_TILE] = b_;
        eval_plan_jet<2>(blob, xn, col);
    } else if (pw == 3) {
        eval_plan_jet<3>(blob, xn, col);
    } else if (pw == 4) {
        eval_plan_jet<4>(blob, xn, col);
    } else if (pw == 5) {
        float a_, b_;
        np_sincos(state(7), a_, b_);
        shr[0 * LIN_TILE] = a_;
        shr[1 * LIN_TILE] = b_;
        np_sincos(state(8), a_, b_);
        shr[2 * LIN_TILE] = a_;
        shr[3 * LIN_TILE] = b_;
        eval_plan_jet<5>(blob, xn, col);
    } else if (pw == 6) {
        eval_plan_jet<6>(blob, xn, col);
    } else {
        eval_plan_jet<7>(blob, xn, col);
    }
}

}  // namespace npf16
