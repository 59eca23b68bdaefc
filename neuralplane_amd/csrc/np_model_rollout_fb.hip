// np_model_rollout_fb.hip — iLQR's forward pass on the flight model: H Euler applications of F16Model.update (reference
// envs/models/F16_model.py:51-67) under the time-varying affine feedback law that np_f16_model_ilqr_backward returns,
//     a_t = abar_t + alpha k_t + K_t (x_t - xbar_t),   x = (s[12], u[0:4] entering the step),
// for L step sizes alpha per problem, as ONE launch (np_f16_model_rollout_feedback).  The action of step t depends on the state the kernel
// has just computed, so this is not an open-loop rollout of given actions; everything else is: the same device functions (control_lag,
// nlplant) in the same order, the same two shapes, the same state carry and recording as np_model_rollout.hip.  A pure function.
//
// The new thing is the feedback record: one problem-step is 84 floats (K 64, k 4, sbar 12, abar 4) where the open-loop kernel reads 4.
//   - output row r is problem r / L, candidate r % L: the candidates of a problem are ADJACENT LANES, so every load of the record hits
//     64 / L distinct addresses per wave, the record's HBM traffic per output row falls with L, and nothing is copied per candidate.
//   - the record does not ride in registers across the net evaluation (the asm phases own s4-s101 and the throughput shape is built for
//     three waves per SIMD): only ubar (the nominal lagged controls, carried beside u) and the next step's abar and k, requested before
//     the nets, cross them.  sbar_t and the 64 planes of K_t are loaded at the head of step t, after the state update that made x_t, and
//     consumed in order, one output's 16 planes at a time, into the two FMA chains of the spelled summation order:
//         c = fma(alpha, k[a], abar[a]);  d_j = x_j - xbar_j;  lo = sum_{j<8} K[a][j] d_j;  hi = sum_{j>=8} K[a][j] d_j  (a product, then
//         FMAs, j ascending);  a_t[a] = c + (lo + hi)
//   - split shape: the mat-vec is split over the eight waves.  Wave w owns planes 8 w .. 8 w + 7 of K_t — output a = w / 2, half w % 2 of
//     its chain — 8 loads per lane instead of 64, and leaves its half-sum in LDS beside the tile's shared scalars; one barrier more per step
//     publishes the eight half-sums, and every wave forms c + (lo + hi) itself.  This is why the order above is two half-chains: both
//     shapes compute the same bits.
//   - the fused cost (optional) accumulates per row in one register; the choice of step size is a butterfly over the L adjacent lanes
//     of a problem (L a power of two: a problem never straddles a wave), in registers.
#include "np_model_rollout_fb.h"

#include "np_f16_device.h"
#include "np_f16_kargs.h"

namespace npf16 {

typedef const FeedbackArgs __attribute__((address_space(4))) *FeedbackArgsC;
typedef const float __attribute__((address_space(4))) *ConstFloats;   // uniform reads of the workspace: scalar loads

// an opaque copy: what is computed from it is computed again, not kept in a register across the net evaluations
__device__ __forceinline__ unsigned fresh(unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
}

constexpr int FB_PARTS = 8;   // split shape: the half-sums of the four outputs, one LDS column per wave

template <int SHAPE>
__global__ __launch_bounds__(SHAPE == ROLLOUT_SPLIT ? ROLLOUT_TILE_SPLIT * ROLLOUT_SPLIT_WAVES : ROLLOUT_TILE_THROUGHPUT)
__attribute__((amdgpu_waves_per_eu((SHAPE == ROLLOUT_SPLIT ? 2 : 3), 8)))
void f16_rollout_fb_kernel(const FeedbackArgs a) {
    constexpr bool SPLIT = SHAPE == ROLLOUT_SPLIT;
    constexpr int TILE = SPLIT ? ROLLOUT_TILE_SPLIT : ROLLOUT_TILE_THROUGHPUT;
    constexpr int WPT = SPLIT ? ROLLOUT_SPLIT_WAVES : 2;
    static_assert(!SPLIT || WPT == FB_PARTS, "one half-sum per wave");
    // coefficient columns, then the partner's normalised inputs (throughput) or the tile's shared scalars and the half-sums (split)
    constexpr int COLS = NUM_LDS_SLOTS + (SPLIT ? NUM_SHARED_SCALARS + FB_PARTS : NUM_NORM_GROUPS);
    __shared__ __attribute__((aligned(16))) float lds[COLS * TILE];
    const int t = SPLIT ? (int)(threadIdx.x % TILE) : (int)threadIdx.x;
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    float *coef = lds + t;
    const long long i = (long long)blockIdx.x * TILE + t;
    const bool valid = i < a.rows;
    const bool writer = valid && (!SPLIT || pw == 0);
    const unsigned r = (unsigned)(valid ? i : a.rows - 1);  // tail lanes shadow the last row; their stores are masked
    FeedbackArgsC ap = (FeedbackArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    // rows of every array are (uniform 64-bit base) + (32-bit byte offset): the host keeps ld0, ld, ld_out and problems * act_row_stride
    // below 2^30 and rows below 2^28 (16 bytes of actions_out per row)
    // Of what is derived from the row only q4 is carried across the net evaluations: the rest is recomputed where it is used (fresh())
    const unsigned q = r / (unsigned)a.n_alpha;
    const unsigned q4 = q * 4u;
    const unsigned src4 = (q / (unsigned)a.fanout) * 4u;
    float s[12], u[4], ub[4];
#pragma unroll
    for (int k = 0; k < 4; k++) ub[k] = at_off(a.u0 + k * a.ld0, src4);
    if (a.s_init) {
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] = at_off(a.s_init + k * a.ld, q4);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = at_off(a.u_init + k * a.ld, q4);
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] = at_off(a.s0 + k * a.ld0, src4);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = ub[k];
    }
    const unsigned act4 = q * (unsigned)a.act_row_stride * 4u;
    float an[4], kn[4];  // step t's abar and k: in flight across step t - 1's net evaluation
#pragma unroll
    for (int k = 0; k < 4; k++) {
        an[k] = at_off(a.actions, act4 + 4u * k);
        kn[k] = at_off(a.k + k * a.ld, q4);
    }

    StateScalars sc;
    if constexpr (!SPLIT) {
        trig_of(s, sc.tr, sc.tt);
        sc.powv = atmos_pow(ap->cfg.af, s[2]);
    }

    float cost = 0.0f;
#pragma nounroll
    for (int step = 0; step < ap->horizon; step++) {
        NP_REREAD_ARGS(ap);
        // ---- the law ----
        const unsigned qv = fresh(q4) >> 2;
        const float alpha = at_off(ap->ws, (r - qv * (unsigned)ap->n_alpha) * 4u);
        float c[4], nom[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            c[k] = fmaf(alpha, kn[k], an[k]);
            float v = an[k];  // the nominal flight's clamped action: what ubar lags
            v = v < -1.0f ? -1.0f : v;
            v = v > 1.0f ? 1.0f : v;
            nom[k] = v;
        }
        // xbar_t: the start row for t = 0, the nominal trajectory's record t - 1 after it; ubar_t is carried
        const float *sb = step == 0 ? ap->s0 : ap->s_traj + (long long)(step - 1) * ap->traj_step_stride;
        const long long sb_ld = step == 0 ? ap->ld0 : ap->ld;
        const unsigned sb4 = step == 0 ? (qv / (unsigned)ap->fanout) * 4u : q4;
        const float *Kt = ap->K + (long long)step * 64 * ap->ld;
        float act[4];
        if constexpr (!SPLIT) {
            float d[16];
#pragma unroll
            for (int j = 0; j < 12; j++) d[j] = s[j] - at_off(sb + j * sb_ld, sb4);
#pragma unroll
            for (int j = 0; j < 4; j++) d[12 + j] = u[j] - ub[j];
#pragma unroll
            for (int o = 0; o < 4; o++) {  // one output's 16 planes at a time: the chains start as the first planes land
                float kk[16];
#pragma unroll
                for (int j = 0; j < 16; j++) kk[j] = at_off(Kt + (16 * o + j) * ap->ld, q4);
                float lo = kk[0] * d[0], hi = kk[8] * d[8];
#pragma unroll
                for (int j = 1; j < 8; j++) {
                    lo = fmaf(kk[j], d[j], lo);
                    hi = fmaf(kk[8 + j], d[8 + j], hi);
                }
                act[o] = c[o] + (lo + hi);
            }
        } else {
            // this wave's half-chain: planes 8 pw .. 8 pw + 7 are K[pw / 2][8 (pw % 2) ..]
            const bool upper = (pw & 1) != 0;
            float d[8];
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = (upper ? s[8 + j] : s[j]) - at_off(sb + (upper ? 8 + j : j) * sb_ld, sb4);
            if (upper) {
#pragma unroll
                for (int j = 0; j < 4; j++) d[4 + j] = u[j] - ub[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) d[4 + j] = s[4 + j] - at_off(sb + (4 + j) * sb_ld, sb4);
            }
            float kk[8];
#pragma unroll
            for (int j = 0; j < 8; j++) kk[j] = at_off(Kt + (8 * pw + j) * ap->ld, q4);
            float half = kk[0] * d[0];
#pragma unroll
            for (int j = 1; j < 8; j++) half = fmaf(kk[j], d[j], half);
            float *parts = coef + (NUM_LDS_SLOTS + NUM_SHARED_SCALARS) * TILE;
            parts[pw * TILE] = half;
            __syncthreads();  // the eight half-sums of this step are in LDS (the last step's were read before its net evaluation's barriers)
#pragma unroll
            for (int o = 0; o < 4; o++) act[o] = c[o] + (parts[(2 * o) * TILE] + parts[(2 * o + 1) * TILE]);
        }
        // ---- F16Model.update (F16_model.py:51-67) ----
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float v = act[k];
            v = v < -1.0f ? -1.0f : v;  // torch.clamp(action, -1, 1); NaN stays NaN
            v = v > 1.0f ? 1.0f : v;
            act[k] = v;
        }
        if (writer) {
            float *ao = ap->actions_out + (long long)step * ap->rows * 4;
            typedef float __attribute__((ext_vector_type(4))) f4;
            f4 v4 = {act[0], act[1], act[2], act[3]};
            at_off(reinterpret_cast<f4 *>(ao), r * 16u) = v4;
        }
        if (ap->cost) {  // the action's terms of this step, k ascending; the state's follow the step
#pragma unroll
            for (int k = 0; k < 4; k++) cost = cost + 0.5f * (ap->h_a[k] * (act[k] * act[k]));
        }
        if (step + 1 < ap->horizon) {  // the next step's abar and k: in flight across this step's net evaluation
            const float *nxt = ap->actions + (long long)(step + 1) * ap->act_step_stride;
            const float *kx = ap->k + (long long)(step + 1) * 4 * ap->ld;
            const unsigned act4 = qv * (unsigned)ap->act_row_stride * 4u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                an[k] = at_off(nxt, act4 + 4u * k);
                kn[k] = at_off(kx + k * ap->ld, q4);
            }
        }
        control_lag(ap->cfg.af, nom, ub);
        control_lag(ap->cfg.af, act, u);
        const AeroWeights wts = {ap->wt.kblob, ap->wt.kblob_dual, ap->wt.pwl, ap->wt.pwl_unnorm, nullptr};
        float k1[12];
        if constexpr (SPLIT) {
            nlplant<true, AB_ALL, TILE, WPT, true, 0>(wts, airframe_via(ap), s, u, sc, coef, false, k1, pw);
            __syncthreads();  // every wave has read the tile's shared scalars before the next step's are written over them
        } else {
            np_sincos(s[5], sc.spsi, sc.cpsi);
            nlplant<true, AB_ALL, TILE, WPT, false, 0, true>(wts, airframe_via(ap), s, u, sc, coef, false, k1, pw);
        }
        NP_REREAD_ARGS(ap);
        const float dt = ap->cfg.dt;
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] = s[k] + dt * k1[k];
        if constexpr (!SPLIT) {
            if (step + 1 < ap->horizon) {  // the next step's carry
                trig_of(s, sc.tr, sc.tt);
                sc.powv = atmos_pow(ap->cfg.af, s[2]);
            }
        }
        // ---- the new trajectory (always recorded: the next backward pass linearises about it) and the state's cost terms ----
        if (writer) {
            float *rec = ap->s_traj_out + (long long)step * 12 * ap->ld_out;
#pragma unroll
            for (int k = 0; k < 12; k++) at_off(rec + k * ap->ld_out, r * 4u) = s[k];
        }
        if (ap->cost && (!SPLIT || pw == 0)) {
            const float *ref = ap->s_ref + (long long)step * 12 * ap->ld;
            ConstFloats hs = (ConstFloats)(ap->ws + FB_WS_ALPHAS + step * 12);
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const float e = s[k] - at_off(ref + k * ap->ld, q4);
                cost = cost + 0.5f * (hs[k] * (e * e));
            }
        }
    }

    NP_REREAD_ARGS(ap);
    if (writer) {
        const unsigned w4 = r * 4u;
#pragma unroll
        for (int k = 0; k < 12; k++) at_off(ap->s_out + k * ap->ld_out, w4) = s[k];
#pragma unroll
        for (int k = 0; k < 4; k++) at_off(ap->u_out + k * ap->ld_out, w4) = u[k];
        // the fifth control is not F16Model.update's business: handed through from the start the row flew from
        at_off(ap->u_out + 4 * ap->ld_out, w4) = ap->u_init ? at_off(ap->u_init + 4 * ap->ld, q4)
                                                            : at_off(ap->u0 + 4 * ap->ld0, ((fresh(q4) >> 2) / (unsigned)ap->fanout) * 4u);
    }
    if (ap->cost && (!SPLIT || pw == 0)) {
        if (valid) at_off(ap->cost, r * 4u) = cost;
        if (ap->best) {
            // the lowest finite cost of the problem's n_alpha adjacent lanes, ties to the lowest candidate: a butterfly in registers.  n_alpha is
            // a power of two and divides the tile, so a problem's lanes are one aligned group of one wave, all valid or all masked
            const float inf = __builtin_inff();
            float cv = (cost - cost == 0.0f) ? cost : inf;
            const int cand = (int)(r - (fresh(q4) >> 2) * (unsigned)ap->n_alpha);
            int idx = cand;
            for (int m = 1; m < ap->n_alpha; m <<= 1) {
                const float oc = __shfl_xor(cv, m, 64);
                const int oi = __shfl_xor(idx, m, 64);
                const bool take = oc < cv || (oc == cv && oi < idx);
                cv = take ? oc : cv;
                idx = take ? oi : idx;
            }
            if (valid && cand == 0) at_off(ap->best, q4) = cv < inf ? idx : -1;
        }
    }
}

hipError_t launch_model_rollout_feedback(int shape, const FeedbackArgs &args, hipStream_t stream) {
    if ((shape != ROLLOUT_THROUGHPUT && shape != ROLLOUT_SPLIT) || args.rows <= 0 || args.horizon < 1 || args.n_alpha < 1 || args.n_alpha > FB_WS_ALPHAS ||
        args.fanout < 1 || args.rows % args.n_alpha != 0)
        return hipErrorInvalidValue;
    const int tile = shape == ROLLOUT_SPLIT ? ROLLOUT_TILE_SPLIT : ROLLOUT_TILE_THROUGHPUT;
    const dim3 grid((unsigned)((args.rows + tile - 1) / tile));
    if (shape == ROLLOUT_SPLIT)
        hipLaunchKernelGGL((f16_rollout_fb_kernel<ROLLOUT_SPLIT>), grid, dim3(ROLLOUT_TILE_SPLIT * ROLLOUT_SPLIT_WAVES), 0, stream, args);
    else
        hipLaunchKernelGGL((f16_rollout_fb_kernel<ROLLOUT_THROUGHPUT>), grid, dim3(ROLLOUT_TILE_THROUGHPUT), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
