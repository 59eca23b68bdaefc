// np_model_mppi.hip — one MPPI iteration on the flight model (np_f16_model_mppi): for P problems, K candidate action sequences each are
// sampled around the problem's nominal plan, flown for H Euler applications of F16Model.update (reference envs/models/F16_model.py:51-67),
// costed, and folded back into one new plan per problem by softmin weights.  Two launches, back to back on the caller's stream.
//
// What the torch route around np_f16_model_rollout writes to memory — the noise [H][P K][4], the candidates [H][P K][4], the trajectory
// [H][12][P K] — never exists here.  The noise is a pure function of (seed, call, row): Philox4x32-10 block 2 of the numerics spec and the
// packed two-pair Box-Muller (np_math.h, np_f16_device.h: the generator of the observation noise, which the oracle restates bit for bit), so
// the rollout makes a row's four normals in registers when it needs them and the re-weighting pass makes them AGAIN, instead of either
// kernel reading what the other wrote.  Between the two kernels goes one float per candidate: its cost.
//
// Kernel 1, f16_mppi_rollout_kernel<SHAPE>: the open-loop rollout (np_model_rollout.hip) in its two shapes, same device functions in the
// same order, same tile, LDS and state carry.  Differences:
//   - no action stream per row.  Output row r is problem r / K, candidate r % K: the candidates of a problem are ADJACENT LANES and read
//     their problem's abar_t, 64 / K distinct addresses per wave.  Step t + 1's abar is requested before step t's net evaluation.
//   - eps is drawn at the head of a step, before the nets, where the asm phases do not yet own the registers.  Nothing of the generator
//     crosses the net evaluation — no Philox state, no counters, no row-derived offset but q * 4 (the rest is recomputed behind an opaque
//     copy, as the feedback rollout does) — except the four normals themselves, which a hold > 1 flies again.
//   - the cost of np_f16_feedback_io (same terms, same order) rides in one accumulator; the row stores 4 bytes at the end, and nothing per
//     step unless actions_out is asked for.
//   - split shape: EVERY wave of a tile draws the row's eps itself.  All eight need the action (each lags the controls its slice of the nets
//     reads), so the alternative is wave 0 publishing four floats per row through LDS and one more barrier per step; a draw is ~150 VALU
//     instructions beside a barrier that idles eight waves in a shape chosen because the launch is latency-bound, and needs no LDS.
//
// Kernel 2, f16_mppi_update_kernel: a wave owns a problem — for K <= 32 it owns 64 / K' of them, K' = K rounded up to a power of two, the
// surplus lanes masked — and its lanes stride over the candidates.  Pass A reads the K costs once: minimum and index by a register
// butterfly, weights, their sum, the normalised weights' sum of squares.  Pass B, per step: each lane makes the eps of its candidates
// again, forms the clamped action, accumulates w * a; a butterfly, and the group's first lane stores 16 bytes.  For K <= 64 a lane has one
// candidate and its weight stays in a register; above that a lane parks its candidates' weights in LDS (its own words: no barrier).
#include "np_model_mppi.h"

#include "np_f16_device.h"
#include "np_f16_kargs.h"

namespace npf16 {

typedef const MppiArgs __attribute__((address_space(4))) *MppiArgsC;
typedef const float __attribute__((address_space(4))) *ConstFloats;   // uniform reads of the workspace: scalar loads

// an opaque copy: what is computed from it is computed again, not kept in a register across the net evaluations
__device__ __forceinline__ unsigned fresh(unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
}

// eps[r][t]: the first four normals of the spec's draw for (seed, call, row) — pairs 0 and 1 of counter block 2, statement for statement
// what add_rng_noise does for o[0..3] at scale 1 on a zero observation.  Candidate 0 of a problem flies the nominal plan: zeros.
__device__ __forceinline__ void mppi_eps(uint64_t seed, uint64_t call, unsigned row, bool nominal, float (&eps)[4]) {
    uint32_t blk[4], k1[3], k2[3];
    rng_block(seed, call, (int64_t)row, 2u, blk);
    noise_block_indices(blk, k1, k2);
    float o[22];
#pragma unroll
    for (int k = 0; k < 22; k++) o[k] = 0.0f;
    add_noise_pairs2(k1[0], k2[0], 0, k1[1], k2[1], 1, 1.0f, o);
#pragma unroll
    for (int k = 0; k < 4; k++) eps[k] = nominal ? 0.0f : o[k];
}

// a_t = clamp(fma(sigma, eps, abar), -1, 1) as torch.clamp has it: NaN stays NaN
__device__ __forceinline__ float mppi_action(float sigma, float eps, float abar) {
    float v = fmaf(sigma, eps, abar);
    v = v < -1.0f ? -1.0f : v;
    v = v > 1.0f ? 1.0f : v;
    return v;
}

template <int SHAPE>
__global__ __launch_bounds__(SHAPE == ROLLOUT_SPLIT ? ROLLOUT_TILE_SPLIT * ROLLOUT_SPLIT_WAVES : ROLLOUT_TILE_THROUGHPUT)
__attribute__((amdgpu_waves_per_eu((SHAPE == ROLLOUT_SPLIT ? 2 : 3), 8)))
void f16_mppi_rollout_kernel(const MppiArgs a) {
    constexpr bool SPLIT = SHAPE == ROLLOUT_SPLIT;
    constexpr int TILE = SPLIT ? ROLLOUT_TILE_SPLIT : ROLLOUT_TILE_THROUGHPUT;
    constexpr int WPT = SPLIT ? ROLLOUT_SPLIT_WAVES : 2;
    // coefficient columns, then the partner's normalised inputs (throughput) or the tile's shared scalars (split): the open-loop rollout's
    constexpr int COLS = NUM_LDS_SLOTS + (SPLIT ? NUM_SHARED_SCALARS : NUM_NORM_GROUPS);
    __shared__ __attribute__((aligned(16))) float lds[COLS * TILE];
    const int t = SPLIT ? (int)(threadIdx.x % TILE) : (int)threadIdx.x;
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    float *coef = lds + t;
    const long long i = (long long)blockIdx.x * TILE + t;
    const bool valid = i < a.rows;
    const bool writer = valid && (!SPLIT || pw == 0);
    const unsigned r = (unsigned)(valid ? i : a.rows - 1);  // tail lanes shadow the last row; their stores are masked
    MppiArgsC ap = (MppiArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    // rows of every array are (uniform 64-bit base) + (32-bit byte offset): the host keeps ld0, ld and problems * act_row_stride below 2^30
    // and rows below 2^28 (16 bytes of actions_out per row).  Of what is derived from the row only q4 is carried across the net evaluations
    const unsigned q4 = (r / (unsigned)a.candidates) * 4u;
    float s[12], u[4];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = at_off(a.s0 + k * a.ld0, q4);
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = at_off(a.u0 + k * a.ld0, q4);
    float an[4];  // step t's abar: in flight across step t - 1's net evaluation
#pragma unroll
    for (int k = 0; k < 4; k++) an[k] = at_off(a.actions, (q4 >> 2) * (unsigned)a.act_row_stride * 4u + 4u * k);

    StateScalars sc;
    if constexpr (!SPLIT) {
        trig_of(s, sc.tr, sc.tt);
        sc.powv = atmos_pow(ap->cfg.af, s[2]);
    }

    float cost = 0.0f, eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int held = 0, draws = 0;
#pragma nounroll
    for (int step = 0; step < ap->horizon; step++) {
        NP_REREAD_ARGS(ap);
        // ---- the candidate's action: a new draw every `hold` steps ----
        const unsigned qv = fresh(q4) >> 2;
        if (held == 0) {
            mppi_eps(ap->seed, ap->call0 + (unsigned)draws, r, r == qv * (unsigned)ap->candidates, eps);
            draws++;
        }
        if (++held == ap->hold) held = 0;
        float act[4];
#pragma unroll
        for (int k = 0; k < 4; k++) act[k] = mppi_action(ap->sigma[k], eps[k], an[k]);
        if (ap->actions_out && writer) {
            float *ao = ap->actions_out + (long long)step * ap->rows * 4;
            typedef float __attribute__((ext_vector_type(4))) f4;
            f4 v4 = {act[0], act[1], act[2], act[3]};
            at_off(reinterpret_cast<f4 *>(ao), r * 16u) = v4;
        }
        // the action's terms of this step, k ascending; the state's follow the step
#pragma unroll
        for (int k = 0; k < 4; k++) cost = cost + 0.5f * (ap->h_a[k] * (act[k] * act[k]));
        if (step + 1 < ap->horizon) {  // the next step's abar: in flight across this step's net evaluation
            const float *nxt = ap->actions + (long long)(step + 1) * ap->act_step_stride;
            const unsigned act4 = qv * (unsigned)ap->act_row_stride * 4u;
#pragma unroll
            for (int k = 0; k < 4; k++) an[k] = at_off(nxt, act4 + 4u * k);
        }
        // ---- F16Model.update (F16_model.py:51-67), as np_model_rollout.hip runs it ----
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
        // ---- the state's cost terms against s_ref[t] ----
        if (!SPLIT || pw == 0) {
            const float *ref = ap->s_ref + (long long)step * 12 * ap->ld;
            ConstFloats hs = (ConstFloats)(ap->ws + step * 12);
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const float e = s[k] - at_off(ref + k * ap->ld, q4);
                cost = cost + 0.5f * (hs[k] * (e * e));
            }
        }
    }

    NP_REREAD_ARGS(ap);
    if (writer) at_off(ap->cost, r * 4u) = cost;
}

// sum / minimum over the `width` adjacent lanes of an aligned group (width a power of two, wave-uniform): every lane ends with the result
__device__ __forceinline__ float group_sum(float v, int width) {
    for (int m = 1; m < width; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(64 * MPPI_UPDATE_WAVES)
void f16_mppi_update_kernel(const MppiArgs a) {
    extern __shared__ float parked[];  // K > 64: [waves][K], a lane's candidates' costs, then their weights
    const int K = a.candidates;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    int width = 64;  // lanes per problem
    if (K <= 32)
        for (width = 1; width < K; width <<= 1) {}
    const bool one = K <= 64;  // one candidate per lane: its cost and weight stay in `mine`
    const long long q = ((long long)blockIdx.x * MPPI_UPDATE_WAVES + wave) * (64 / width) + lane / width;
    const int c0 = lane & (width - 1);
    const bool live = q < a.problems && c0 < K;  // masked lanes carry neutral values through the butterflies; they load and store nothing
    float *park = parked + (one ? 0 : wave * K);
    const float *cost = a.cost + q * K;
    const float inf = __builtin_inff();

    // ---- pass A: the lowest finite cost and its index (ties to the lowest), the weights, their sum, the sum of squares ----
    float mine = inf, cmin = inf;
    int idx = 0x7FFFFFFF;
    for (int c = c0; live && c < K; c += 64) {
        const float v = cost[c];
        if (one) mine = v;
        else park[c] = v;
        const float f = (v - v == 0.0f) ? v : inf;
        if (f < cmin) {  // c ascends: the first of equals stays
            cmin = f;
            idx = c;
        }
    }
    for (int m = 1; m < width; m <<= 1) {
        const float oc = __shfl_xor(cmin, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        const bool take = oc < cmin || (oc == cmin && oi < idx);
        cmin = take ? oc : cmin;
        idx = take ? oi : idx;
    }
    const bool any = cmin < inf;  // no finite candidate: all the weight on candidate 0, the clamped nominal
    float sum = 0.0f;
    for (int c = c0; live && c < K; c += 64) {
        const float v = one ? mine : park[c];
        float w = 0.0f;
        if (any) {
            if (v - v == 0.0f) w = np_exp((cmin - v) / a.temperature);
        } else if (c == 0) {
            w = 1.0f;
        }
        if (one) mine = w;
        else park[c] = w;
        sum = sum + w;
    }
    if (!live) mine = 0.0f;
    sum = group_sum(sum, width);  // >= 1: the cheapest candidate's weight is exp(0)
    float sq = 0.0f;
    for (int c = c0; live && c < K; c += 64) {
        const float w = (one ? mine : park[c]) / sum;
        if (one) mine = w;
        else park[c] = w;
        sq = sq + w * w;
    }
    sq = group_sum(sq, width);
    if (live && c0 == 0) {
        if (a.best) a.best[q] = any ? idx : -1;
        if (a.ess) a.ess[q] = any ? 1.0f / sq : 0.0f;
    }

    // ---- pass B: plan_out[t][q] = sum_c w_c a[q K + c][t], the actions made again from the counters ----
    const unsigned row0 = (unsigned)(live ? q * K : 0);
    float next[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // step t + 1's abar is requested before step t's draws: its latency hides behind them
    if (live) {
#pragma unroll
        for (int k = 0; k < 4; k++) next[k] = a.actions[q * a.act_row_stride + k];
    }
    for (int t = 0; t < a.horizon; t++) {
        const uint64_t call = a.call0 + (unsigned)(t / a.hold);
        float abar[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; k++) abar[k] = next[k];
        if (live && t + 1 < a.horizon) {
            const float *ab = a.actions + (long long)(t + 1) * a.act_step_stride + q * a.act_row_stride;
#pragma unroll
            for (int k = 0; k < 4; k++) next[k] = ab[k];
        }
        for (int c = c0; live && c < K; c += 64) {
            const float w = one ? mine : park[c];
            float eps[4];
            mppi_eps(a.seed, call, row0 + (unsigned)c, c == 0, eps);
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] = fmaf(w, mppi_action(a.sigma[k], eps[k], abar[k]), acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] = group_sum(acc[k], width);
        if (live && c0 == 0) {
            typedef float __attribute__((ext_vector_type(4))) f4;
            f4 v4 = {acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f4 *>(a.plan_out + ((long long)t * a.problems + q) * 4) = v4;
        }
    }
}

hipError_t launch_model_mppi(int shape, const MppiArgs &args, hipStream_t stream) {
    if ((shape != ROLLOUT_THROUGHPUT && shape != ROLLOUT_SPLIT) || args.problems < 1 || args.horizon < 1 || args.hold < 1 || args.candidates < 1 ||
        args.candidates > MPPI_MAX_CANDIDATES || args.rows != (long long)args.problems * args.candidates)
        return hipErrorInvalidValue;
    const int tile = shape == ROLLOUT_SPLIT ? ROLLOUT_TILE_SPLIT : ROLLOUT_TILE_THROUGHPUT;
    const dim3 grid((unsigned)((args.rows + tile - 1) / tile));
    if (shape == ROLLOUT_SPLIT)
        hipLaunchKernelGGL((f16_mppi_rollout_kernel<ROLLOUT_SPLIT>), grid, dim3(ROLLOUT_TILE_SPLIT * ROLLOUT_SPLIT_WAVES), 0, stream, args);
    else
        hipLaunchKernelGGL((f16_mppi_rollout_kernel<ROLLOUT_THROUGHPUT>), grid, dim3(ROLLOUT_TILE_THROUGHPUT), 0, stream, args);
    if (const hipError_t e = hipGetLastError()) return e;
    const int K = args.candidates;
    int width = 64;
    if (K <= 32)
        for (width = 1; width < K; width <<= 1) {}
    const long long per_group = (long long)MPPI_UPDATE_WAVES * (64 / width);
    const dim3 grid2((unsigned)((args.problems + per_group - 1) / per_group));
    const size_t lds = K > 64 ? sizeof(float) * MPPI_UPDATE_WAVES * (size_t)K : 0;
    hipLaunchKernelGGL(f16_mppi_update_kernel, grid2, dim3(64 * MPPI_UPDATE_WAVES), lds, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
