// np_model_trim.hip — batched trim: a damped Newton solve for a steady flight condition, per row, run to convergence in ONE launch
// (np_f16_model_trim).  Per row, with z = (s[0..11], u[0..3]) and m <= 12 unknowns q that move z along the columns of D [16][m]:
//     r(z) = (xdot(z) - tgt)[rows],   phi = sum_i (r_i / scale[rows[i]])^2,   J = [A | B][rows, :] D,   J delta = -r,   z+ = clamp(z + D delta)
// xdot, A and B are F16Dynamics.nlplant's and its analytic Jacobian, exactly as np_model_linearize.hip computes them (np_model_jets.h).
// A pure function: nothing of the context is written.
//
// Schedule: the linearisation tile made persistent over the Newton loop.  One lane = one row of a 64-row tile, eight waves share the tile,
// the weight blob sits in LDS once per workgroup, a workgroup walks the tiles blockIdx.x, + gridDim.x, ...  Per tile and trip p = 0..max_iters:
//   - pass A at the row's trial point zt (LDS): phase 1 = the 110 columns by PLAN8_LIN and the 12 shared scalars; phase 2 = every wave pushes
//     its two directions through nlplant_jets<2> and, instead of storing 12 floats per column to HBM, puts the m selected rows of each
//     column into the row's G [m][14] in LDS; wave 0 adds r.  Nothing but the final result touches HBM.
//   - wave 0, one lane per row: the Armijo test of the full step, phi(zt) <= (1 - 2c) phi(z) (c = 1e-4; the trip-0 point and a point the
//     backtracking chose are accepted by definition), convergence phi <= tol^2, then J = G D in direction order, rows divided by their
//     scale, fp32 LU with partial pivoting in place in LDS, run-time m, delta, D delta and the clamped next trial point.  The test is free:
//     phi(zt) is pass A's own xdot, and G is already the next step's Jacobian.
//   - if any row of the tile failed the test (a workgroup-uniform vote through LDS): backtracking.  Step sizes 2^-1 .. 2^-8, largest first:
//     the eight waves evaluate the nets BY VALUE (eval_plan_val: no tangent chains, the same split) at clamp(z + alpha D delta), wave 0
//     runs the equations of motion by value and gives each failing row the first alpha with phi_alpha <= (1 - 2 c alpha) phi; the loop
//     ends as soon as no row of the tile is still looking.  A row that finds none stalls.  Rows that passed are not touched.
// A row's path depends on nothing but the row: every trip evaluates every unfinished row at its own trial point, whatever its neighbours do;
// only the number of backtracking passes a tile runs depends on the tile.  iters[row] = the passes A the row used after the first.
//
// BARRIERS.  Finished rows (converged, stalled, singular, non-finite, out of trips) are masked, never exited: every __syncthreads() below
// sits in control flow that depends only on kernel arguments and on flags that ONE lane wrote to LDS before the preceding barrier and
// that all eight waves read after it (readfirstlane), so all eight waves reach every barrier and the trip counts (at most max_iters + 1
// trips, at most eight backtracking passes per trip) are workgroup-uniform.  No barrier is inside per-row (divergent) code.
//
// Matrix instructions are not used.  The nets: for the reasons at the head of np_model_linearize.hip.  The solve: it is 64 independent
// m x m systems (m <= 12, run-time) with per-row pivoting — a lane's private row exchanges, nothing an MFMA tile expresses.
#include "np_model_trim.h"

#include "np_model_jets.h"

namespace npf16 {

constexpr int TRIM_G_STRIDE = 15;                       // per residual: 14 directions (then J's m columns), and r in entry 14
constexpr int TG_R = 14, TG_X = 13;                     // entry 13: the column's largest element, then the solution
constexpr int TRIM_ROW_COLS = TRIM_MAX_M * TRIM_G_STRIDE + 3 * TRIM_Z + 9;   // G, z, zt, dl, phi / status / iters / forced / needbt / finite / row offset / row is real / backtracks
constexpr int TRIM_LDS_FLOATS = LIN_LDS_FLOATS + TRIM_ROW_COLS * LIN_TILE + 4;
static_assert(TRIM_LDS_FLOATS * sizeof(float) <= 160 * 1024, "fits a CU's LDS");
static_assert(NUM_LIN_DIRS == 14 && D_T + 2 == 12, "direction d moves z[d + 2]");

typedef const TrimArgs __attribute__((address_space(4))) *TrimArgsC;

// The workgroup's LDS: the blob, then this lane's columns (stride LIN_TILE) at compile-time places behind ONE index: fourteen separate
// pointers would be fourteen VGPRs live across both phases.
struct TrimLds {
    float *blob;   // the __shared__ array itself: every place below stays an LDS address for the compiler
    int t;         // this lane
    // an opaque statement per phase: the places derived from `t` are made again behind it, not kept in registers across the nets
    __device__ __forceinline__ void fence() { asm volatile("" : "+v"(t)); }
    __device__ __forceinline__ float *at(int cols) const { return blob + (KBLOB_FLOATS + cols * LIN_TILE) + t; }
    __device__ __forceinline__ float *col() const { return at(0); }
    __device__ __forceinline__ float *shr() const { return at(LIN_COLS); }
    __device__ __forceinline__ float *G() const { return at(LIN_COLS + NUM_SHARED_SCALARS); }
    __device__ __forceinline__ float *z() const { return at(LIN_COLS + NUM_SHARED_SCALARS + TRIM_MAX_M * TRIM_G_STRIDE); }
    __device__ __forceinline__ float *zt() const { return z() + TRIM_Z * LIN_TILE; }
    __device__ __forceinline__ float *dl() const { return z() + 2 * TRIM_Z * LIN_TILE; }
    __device__ __forceinline__ float *phi() const { return z() + 3 * TRIM_Z * LIN_TILE; }
    __device__ __forceinline__ int *stat() const { return (int *)(phi() + LIN_TILE); }
    __device__ __forceinline__ int *iters() const { return (int *)(phi() + 2 * LIN_TILE); }
    __device__ __forceinline__ int *forced() const { return (int *)(phi() + 3 * LIN_TILE); }
    __device__ __forceinline__ int *needbt() const { return (int *)(phi() + 4 * LIN_TILE); }
    __device__ __forceinline__ int *finite() const { return (int *)(phi() + 5 * LIN_TILE); }
    // the row's byte offset in a row-indexed array and whether the lane has a row of its own: read back where needed, not kept in registers
    __device__ __forceinline__ unsigned *row4() const { return (unsigned *)(phi() + 6 * LIN_TILE); }
    __device__ __forceinline__ int *valid() const { return (int *)(phi() + 7 * LIN_TILE); }
    __device__ __forceinline__ int *nbt() const { return (int *)(phi() + 8 * LIN_TILE); }   // full steps of the row the Armijo test refused
    // [0] some row asks for backtracking, [1] some row is unfinished
    __device__ __forceinline__ int *flags() const { return (int *)(blob + LIN_LDS_FLOATS + TRIM_ROW_COLS * LIN_TILE); }
};

__device__ __forceinline__ float trim_clamp(float v, float lo, float hi) {
    v = v < lo ? lo : v;   // NaN stays NaN
    return v > hi ? hi : v;
}

// Phase 1 at the point pt(k) = entry k of z.  The chain has twins, np_model_jets.h::lin_phase1 and np_model_linearize.hip's: which wave
// writes which shared scalar must stay the same in all of them.  TAN = false: the nets by value only.
template <bool TAN, class Pt>
__device__ __forceinline__ bool trim_phase1(int pw, TrimArgsC ap, TrimLds L, Pt pt) {
    L.fence();
    const float r2d = (float)(180.0 / 3.141592653589793);
    const float alpha = pt(7) * r2d, beta = pt(8) * r2d, el = pt(13);
    const float chk = ((alpha - alpha) + (beta - beta)) + (el - el);  // non-finite inputs poison every coefficient (numerics spec)
    float xn[NUM_NORM_GROUPS];
#pragma unroll
    for (int gi = 0; gi < NUM_NORM_GROUPS; gi++) {
        const float v = (gi <= G_A_RUD) ? alpha : (gi <= G_B_O ? beta : el);
        const float *h = L.blob + KBLOB_NORM_STRIDE * gi;  // (mean, sigma, RN(1 / sigma))
        xn[gi] = np_divc(v - h[0], h[1], h[2]);
    }
    float *shr = L.shr(), *col = L.col();
#define NPF16_PLAN(W)                                     \
    do {                                                  \
        if constexpr (TAN) eval_plan_jet<W>(L.blob, xn, col); \
        else eval_plan_val<W>(L.blob, xn, col);           \
    } while (0)
    if (pw == 0) {
        float a_, b_, c_;
        np_sincostan(pt(4), a_, b_, c_);
        shr[4 * LIN_TILE] = a_;
        shr[5 * LIN_TILE] = b_;
        shr[8 * LIN_TILE] = c_;
        np_sincos(pt(3), a_, b_);
        shr[6 * LIN_TILE] = a_;
        shr[7 * LIN_TILE] = b_;
        shr[11 * LIN_TILE] = atmos_pow(ap->af, pt(2));
        NPF16_PLAN(0);
    } else if (pw == 1) {
        NPF16_PLAN(1);
    } else if (pw == 2) {
        float a_, b_;
        np_sincos(pt(5), a_, b_);
        shr[9 * LIN_TILE] = a_;
        shr[10 * LIN_TILE] = b_;
        NPF16_PLAN(2);
    } else if (pw == 3) {
        NPF16_PLAN(3);
    } else if (pw == 4) {
        NPF16_PLAN(4);
    } else if (pw == 5) {
        float a_, b_;
        np_sincos(pt(7), a_, b_);
        shr[0 * LIN_TILE] = a_;
        shr[1 * LIN_TILE] = b_;
        np_sincos(pt(8), a_, b_);
        shr[2 * LIN_TILE] = a_;
        shr[3 * LIN_TILE] = b_;
        NPF16_PLAN(5);
    } else if (pw == 6) {
        NPF16_PLAN(6);
    } else {
        NPF16_PLAN(7);
    }
#undef NPF16_PLAN
    return chk == chk;
}

// r of the selected rows -> G[.][TG_R], from xdot's values (wave 0)
template <int N>
__device__ __forceinline__ void trim_store_r(TrimArgsC ap, TrimLds L, const Jet<N> (&xd)[12]) {
    const unsigned r4 = L.row4()[0];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const int slot = ap->slot_of[k];
        if (slot < 0) continue;  // wave-uniform
        L.G()[(slot * TRIM_G_STRIDE + TG_R) * LIN_TILE] = ap->tgt ? xd[k].v - at_off(ap->tgt + k * ap->ld0, r4) : xd[k].v;
    }
}

// phi = sum_i (r_i / scale)^2, i ascending, one chain (wave 0, one lane per row)
__device__ __forceinline__ float trim_merit(TrimArgsC ap, TrimLds L) {
    float phi = 0.0f;
    for (int i = 0; i < ap->m; i++) {
        const float q = L.G()[(i * TRIM_G_STRIDE + TG_R) * LIN_TILE] / ap->scale[ap->row_of[i]];
        phi = fmaf(q, q, phi);
    }
    return phi;
}

// J = G D (direction order, one chain per element), rows over their scale; LU with partial pivoting in place; delta; dl = D delta and the
// next trial point.  One lane per row; returns the row's status.
__device__ __forceinline__ int trim_solve(TrimArgsC ap, TrimLds L) {
    const int m = ap->m;
    float *G = L.G();
    for (int i = 0; i < m; i++) {
        float g[NUM_LIN_DIRS];
#pragma unroll
        for (int d = 0; d < NUM_LIN_DIRS; d++) g[d] = G[(i * TRIM_G_STRIDE + d) * LIN_TILE];
        const float sc = ap->scale[ap->row_of[i]];
        for (int j = 0; j < m; j++) {
            float acc = g[0] * ap->D[2][j];
#pragma unroll
            for (int d = 1; d < NUM_LIN_DIRS; d++) acc = fmaf(g[d], ap->D[d + 2][j], acc);
            G[(i * TRIM_G_STRIDE + j) * LIN_TILE] = acc / sc;
        }
        G[(i * TRIM_G_STRIDE + TG_R) * LIN_TILE] = -(G[(i * TRIM_G_STRIDE + TG_R) * LIN_TILE] / sc);
    }
    for (int j = 0; j < m; j++) {   // the largest element of each column: what a pivot is measured against
        float cm = 0.0f;
        for (int i = 0; i < m; i++) {
            const float v = fabsf(G[(i * TRIM_G_STRIDE + j) * LIN_TILE]);
            cm = (v > cm || v != v) ? v : cm;
        }
        if (!(cm - cm == 0.0f)) return TRIM_NONFINITE;
        G[(j * TRIM_G_STRIDE + TG_X) * LIN_TILE] = cm;
    }
    for (int c = 0; c < m; c++) {
        int pr = c;
        float pm = fabsf(G[(c * TRIM_G_STRIDE + c) * LIN_TILE]);
        for (int i = c + 1; i < m; i++) {
            const float v = fabsf(G[(i * TRIM_G_STRIDE + c) * LIN_TILE]);
            if (v > pm) {
                pm = v;
                pr = i;
            }
        }
        if (!(pm > 9.5367431640625e-7f * G[(c * TRIM_G_STRIDE + TG_X) * LIN_TILE])) return TRIM_SINGULAR;   // 2^-20
        if (pr != c) {
            for (int j = c; j < m; j++) {
                const float a = G[(c * TRIM_G_STRIDE + j) * LIN_TILE];
                G[(c * TRIM_G_STRIDE + j) * LIN_TILE] = G[(pr * TRIM_G_STRIDE + j) * LIN_TILE];
                G[(pr * TRIM_G_STRIDE + j) * LIN_TILE] = a;
            }
            const float a = G[(c * TRIM_G_STRIDE + TG_R) * LIN_TILE];
            G[(c * TRIM_G_STRIDE + TG_R) * LIN_TILE] = G[(pr * TRIM_G_STRIDE + TG_R) * LIN_TILE];
            G[(pr * TRIM_G_STRIDE + TG_R) * LIN_TILE] = a;
        }
        const float piv = G[(c * TRIM_G_STRIDE + c) * LIN_TILE];
        for (int i = c + 1; i < m; i++) {
            const float f = G[(i * TRIM_G_STRIDE + c) * LIN_TILE] / piv;
            for (int j = c + 1; j < m; j++)
                G[(i * TRIM_G_STRIDE + j) * LIN_TILE] = fmaf(-f, G[(c * TRIM_G_STRIDE + j) * LIN_TILE], G[(i * TRIM_G_STRIDE + j) * LIN_TILE]);
            G[(i * TRIM_G_STRIDE + TG_R) * LIN_TILE] = fmaf(-f, G[(c * TRIM_G_STRIDE + TG_R) * LIN_TILE], G[(i * TRIM_G_STRIDE + TG_R) * LIN_TILE]);
        }
    }
    for (int c = m - 1; c >= 0; c--) {   // the pivots' column maxima are spent: entry TG_X takes the solution
        float v = G[(c * TRIM_G_STRIDE + TG_R) * LIN_TILE];
        for (int j = c + 1; j < m; j++) v = fmaf(-G[(c * TRIM_G_STRIDE + j) * LIN_TILE], G[(j * TRIM_G_STRIDE + TG_X) * LIN_TILE], v);
        G[(c * TRIM_G_STRIDE + TG_X) * LIN_TILE] = v / G[(c * TRIM_G_STRIDE + c) * LIN_TILE];
    }
    float chk = 0.0f;
    for (int e = 0; e < TRIM_Z; e++) {
        float acc = 0.0f;
        for (int j = 0; j < m; j++) acc = fmaf(ap->D[e][j], G[(j * TRIM_G_STRIDE + TG_X) * LIN_TILE], acc);
        L.dl()[e * LIN_TILE] = acc;
        L.zt()[e * LIN_TILE] = trim_clamp(L.z()[e * LIN_TILE] + acc, ap->lo[e], ap->hi[e]);
        chk += acc - acc;
    }
    return chk == 0.0f ? TRIM_RUNNING : TRIM_NONFINITE;
}

// This wave's directions, as in the linearisation: wave 0 the first (and xdot), waves 1..6 two each, wave 7 the last.  Made again per pass
// behind an opaque statement: left loop-invariant, the 0 / 1 seeds nlplant_jets derives from them (two per input) are hoisted out of the
// Newton loop and stay in VGPRs across the nets.
#define TRIM_DIRS(pw)          \
    int w_ = (pw);             \
    asm volatile("" : "+s"(w_)); \
    const int dir[2] = {w_ == 0 ? 0 : 2 * w_ - 1, (w_ == 0 || w_ == LIN_WAVES - 1) ? -1 : 2 * w_}

// Pass A at the row's trial point zt: the columns, then this wave's directions into G and (wave 0) r.  Two barriers, reached by
// every wave.  The arguments are read again behind an opaque statement per phase (np_model_linearize.hip)
__device__ __forceinline__ void trim_pass_a(int pw, TrimArgsC ap, TrimLds L) {
    const float qnan = __builtin_nanf("");
    __syncthreads();  // the blob and the point are there; every wave has read the previous pass's columns
    NP_REREAD_ARGS(ap);
    const bool ok = trim_phase1<true>(pw, ap, L, [&](int k) { return L.zt()[k * LIN_TILE]; });
    __syncthreads();  // all 110 columns and the 12 shared scalars are complete
    NP_REREAD_ARGS(ap);
    L.fence();
    TRIM_DIRS(pw);
    const float *P = L.zt();
    float s[12], u[4];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = P[k * LIN_TILE];
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = P[(12 + k) * LIN_TILE];
    Jet<2> xd[12];
    nlplant_jets<2>(ap->af, s, u, L.shr(), L.col(), dir, ok, xd);
    if (pw == 0) trim_store_r<2>(ap, L, xd);
#pragma unroll
    for (int n = 0; n < 2; n++) {
        if (dir[n] < 0) continue;  // wave-uniform
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int slot = ap->slot_of[k];
            if (slot < 0) continue;  // wave-uniform
            L.G()[(slot * TRIM_G_STRIDE + dir[n]) * LIN_TILE] = (ok || k < 6) ? xd[k].d[n] : qnan;  // as the linearisation stores them
        }
    }
}

// built for two waves per SIMD: one eight-wave workgroup per CU (blob, columns, G and the iterates take 147 KB of its LDS)
__global__ __launch_bounds__(LIN_TILE * LIN_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_trim_kernel(const TrimArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[TRIM_LDS_FLOATS];
    const int t = (int)(threadIdx.x % LIN_TILE);
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LIN_TILE));
    TrimLds L = {lds, t};

    {  // the weight blob, once per workgroup: 16 bytes per thread and turn
        typedef const f32x4 __attribute__((address_space(1))) *gv4;
        const gv4 src = (gv4)(unsigned long long)a.kblob;
        f32x4 *dst = (f32x4 *)L.blob;
        for (int k = (int)threadIdx.x; k < KBLOB_FLOATS / 4; k += LIN_TILE * LIN_WAVES) dst[k] = src[k];
    }

    const float qnan = __builtin_nanf("");
    // the launch's arguments are read through the kernel-argument segment behind an opaque statement per phase (np_model_linearize.hip)
    TrimArgsC ap = (TrimArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    const long long tiles = (a.rows + LIN_TILE - 1) / LIN_TILE;
#pragma nounroll
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        NP_REREAD_ARGS(ap);

        __syncthreads();  // every wave is done with the previous tile's iterates
        {
            const long long i = tile * LIN_TILE + t;
            const bool valid = i < ap->rows;
            const unsigned r4 = (unsigned)(valid ? i : ap->rows - 1) * 4u;  // tail lanes shadow the last row; their stores are masked
#pragma unroll
            for (int n = 0; n < 2; n++) {  // the start: wave w brings entries 2 w and 2 w + 1 of z
                const int e = 2 * pw + n;
                const float v = e < 12 ? at_off(ap->s0 + e * ap->ld0, r4) : at_off(ap->u0 + (e - 12) * ap->ld0, r4);
                L.z()[e * LIN_TILE] = v;
                L.zt()[e * LIN_TILE] = v;
                L.dl()[e * LIN_TILE] = 0.0f;
            }
            if (pw == 0) {
                L.row4()[0] = r4;
                L.valid()[0] = valid ? 1 : 0;
                L.phi()[0] = 0.0f;
                L.stat()[0] = TRIM_RUNNING;
                L.iters()[0] = 0;
                L.forced()[0] = 0;
                L.needbt()[0] = 0;
                L.nbt()[0] = 0;
            }
        }

#pragma nounroll
        for (int p = 0; p <= ap->max_iters; p++) {
            trim_pass_a(pw, ap, L);
            __syncthreads();  // G and r of the trial points are complete

            NP_REREAD_ARGS(ap);
            if (pw == 0) {  // one lane per row: test, accept, converge, solve
                int st = L.stat()[0];
                bool nb = false;
                if (st == TRIM_RUNNING) {
                    const float pt = trim_merit(ap, L);
                    L.iters()[0] = p;
                    bool acc = true;
                    if (p == 0) {
                        if (!(pt - pt == 0.0f)) {
                            st = TRIM_NONFINITE;
                            L.phi()[0] = pt;
                        }
                    } else if (!L.forced()[0]) {
                        acc = pt <= (1.0f - 2.0e-4f) * L.phi()[0];
                    }
                    L.forced()[0] = 0;
                    if (st == TRIM_RUNNING && !acc) {
                        if (p == ap->max_iters) st = TRIM_ITER_LIMIT;
                        else {
                            nb = true;
                            L.nbt()[0] += 1;
                        }
                    } else if (st == TRIM_RUNNING) {
                        for (int e = 0; e < TRIM_Z; e++) L.z()[e * LIN_TILE] = L.zt()[e * LIN_TILE];
                        L.phi()[0] = pt;
                        if (pt <= ap->tol2) st = TRIM_CONVERGED;
                        else if (p == ap->max_iters) st = TRIM_ITER_LIMIT;
                        else st = trim_solve(ap, L);
                    }
                    L.stat()[0] = st;
                    L.needbt()[0] = nb ? 1 : 0;
                    L.finite()[0] = 0;
                }
                const bool any_bt = __ballot(nb) != 0, any_run = __ballot(st == TRIM_RUNNING) != 0;
                if (t == 0) {
                    L.flags()[0] = any_bt ? 1 : 0;
                    L.flags()[1] = any_run ? 1 : 0;
                }
            }
            __syncthreads();  // the votes are in
            const int vote_bt = __builtin_amdgcn_readfirstlane(L.flags()[0]);
            int vote_run = __builtin_amdgcn_readfirstlane(L.flags()[1]);

            if (vote_bt) {  // workgroup-uniform
#pragma nounroll
                for (int k = 0; k < TRIM_BT_STEPS; k++) {
                    const float alpha = __builtin_ldexpf(1.0f, -(k + 1));
                    __syncthreads();  // every wave has read the votes and the previous pass's columns
                    NP_REREAD_ARGS(ap);
                    auto pt = [&](int e) { return trim_clamp(L.z()[e * LIN_TILE] + alpha * L.dl()[e * LIN_TILE], ap->lo[e], ap->hi[e]); };
                    const bool ok = trim_phase1<false>(pw, ap, L, pt);
                    __syncthreads();  // the 42 values and the 12 shared scalars are complete
                    if (pw == 0) {
                        float s[12], u[4];
#pragma unroll
                        for (int e = 0; e < 12; e++) s[e] = pt(e);
#pragma unroll
                        for (int e = 0; e < 4; e++) u[e] = pt(12 + e);
                        const int none[1] = {-1};
                        Jet<1> xd[12];
                        nlplant_jets<1>(ap->af, s, u, L.shr(), L.col(), none, ok, xd);
                        bool nb = L.needbt()[0] != 0;
                        if (nb) {
                            trim_store_r<1>(ap, L, xd);   // the row's G is spent: its trial point was refused
                            const float pa = trim_merit(ap, L);
                            if (pa - pa == 0.0f) L.finite()[0] = 1;
                            if (pa <= (1.0f - 2.0e-4f * alpha) * L.phi()[0]) {
                                for (int e = 0; e < TRIM_Z; e++) L.zt()[e * LIN_TILE] = pt(e);
                                L.forced()[0] = 1;
                                L.needbt()[0] = 0;
                                nb = false;
                            }
                        }
                        const bool more = __ballot(nb) != 0;
                        if (t == 0) L.flags()[0] = more ? 1 : 0;
                    }
                    __syncthreads();  // the vote is in
                    if (!__builtin_amdgcn_readfirstlane(L.flags()[0])) break;  // workgroup-uniform
                }
                __syncthreads();  // every wave has read the last vote
                if (pw == 0) {  // rows no step size served: stalled (no finite phi at all: non-finite)
                    int st = L.stat()[0];
                    if (L.needbt()[0]) {
                        st = L.finite()[0] ? TRIM_STALLED : TRIM_NONFINITE;
                        L.stat()[0] = st;
                        L.needbt()[0] = 0;
                    }
                    const bool any_run = __ballot(st == TRIM_RUNNING) != 0;
                    if (t == 0) L.flags()[1] = any_run ? 1 : 0;
                }
                __syncthreads();
                vote_run = __builtin_amdgcn_readfirstlane(L.flags()[1]);
            }
            if (!vote_run) break;  // workgroup-uniform: every row of the tile has its status
        }

        // ---- the returned point: wave w stores entries 2 w and 2 w + 1 of z, wave 0 the row's res / iters / status ----
        NP_REREAD_ARGS(ap);
        L.fence();
        const bool valid = L.valid()[0] != 0;
        const unsigned r4 = L.row4()[0];
        if (valid) {
#pragma unroll
            for (int n = 0; n < 2; n++) {
                const int e = 2 * pw + n;
                if (e < 12) at_off(ap->s + e * ap->ld_out, r4) = L.z()[e * LIN_TILE];
                else at_off(ap->u + (e - 12) * ap->ld_out, r4) = L.z()[e * LIN_TILE];
            }
            if (pw == LIN_WAVES - 1) at_off(ap->u + 4 * ap->ld_out, r4) = at_off(ap->u0 + 4 * ap->ld0, r4);  // lef is handed through
            if (pw == 0) {
                at_off(ap->res, r4) = sqrtf(L.phi()[0]);
                at_off(ap->iters, r4) = L.iters()[0];
                at_off(ap->status, r4) = L.stat()[0];
                if (ap->backtracks) at_off(ap->backtracks, r4) = L.nbt()[0];
            }
        }

        if (ap->A || ap->xdot) {  // workgroup-uniform: one closing pass A at the returned point, stored as the linearisation stores it
            __syncthreads();
            NP_REREAD_ARGS(ap);
            TRIM_DIRS(pw);
            const float *P = L.z();
            const bool ok = trim_phase1<true>(pw, ap, L, [&](int k) { return P[k * LIN_TILE]; });
            __syncthreads();
            NP_REREAD_ARGS(ap);
            float s[12], u[4];
#pragma unroll
            for (int k = 0; k < 12; k++) s[k] = P[k * LIN_TILE];
#pragma unroll
            for (int k = 0; k < 4; k++) u[k] = P[(12 + k) * LIN_TILE];
            Jet<2> xd[12];
            nlplant_jets<2>(ap->af, s, u, L.shr(), L.col(), dir, ok, xd);
            if (valid) {
                if (pw == 0 && ap->xdot) {
#pragma unroll
                    for (int k = 0; k < 12; k++) at_off(ap->xdot + k * ap->ld_out, r4) = xd[k].v;
                }
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    if (dir[n] < 0 || !ap->A) continue;  // wave-uniform; xdot alone: nothing of A and B is stored
                    const bool in_a = dir[n] < D_T;
                    float *base = in_a ? ap->A + (long long)(dir[n] + 2) * ap->ld_out : ap->B + (long long)(dir[n] - D_T) * ap->ld_out;
                    const long long plane = (in_a ? 12 : 4) * ap->ld_out;
#pragma unroll
                    for (int k = 0; k < 12; k++) at_off(base + k * plane, r4) = (ok || k < 6) ? xd[k].d[n] : qnan;
                }
                if (pw == LIN_WAVES - 1 && ap->A) {  // nothing depends on npos and epos
#pragma unroll
                    for (int k = 0; k < 12; k++) {
                        at_off(ap->A + (long long)(k * 12) * ap->ld_out, r4) = (ok || k < 6) ? 0.0f : qnan;
                        at_off(ap->A + (long long)(k * 12 + 1) * ap->ld_out, r4) = (ok || k < 6) ? 0.0f : qnan;
                    }
                }
            }
        }
    }
}

hipError_t launch_model_trim(int groups, const TrimArgs &args, hipStream_t stream) {
    if (groups < 1 || args.rows < 1 || args.m < 1 || args.m > TRIM_MAX_M || args.max_iters < 0 || args.max_iters > TRIM_MAX_ITERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_trim_kernel, dim3((unsigned)groups), dim3(LIN_TILE * LIN_WAVES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
