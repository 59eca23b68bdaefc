// np_model_rollout.hip — open-loop model rollouts: H applications of F16Model.update (reference envs/models/F16_model.py:51-67: clamp,
// first-order control lag, one integrator step) to a caller-supplied action sequence, as ONE launch (np_f16_model_rollout).
//
// What a look-ahead (MPC, MPPI, a shooting planner) writes as `for t in range(H): model.update(a[t])` on a copy of the state is here a
// pure function of (state, controls, actions): no random numbers, no observation, reward or termination, no auto-reset, and nothing of
// the context is written — not its state, flags, counters, targets or cross-step coefficient cache.  Bit-identical to H launches of
// np_f16_step with inner_step = NP_INNER_UPDATE_ONLY: the same device functions (np_f16_device.h) on the same inputs in the same order.
//
// Schedule (one lane = one output row; a row's 12 states and 5 controls stay in registers for all H steps):
//   - HBM per row: one read of the start state (output row r reads input row r / fanout: K candidates of one aircraft share its lines in
//     cache), 16 bytes of action per step, the recorded states if asked for, one write of the end state and controls.
//   - step t + 1's action is requested before step t's net evaluation starts, so its latency hides behind the 42 nets; nothing waits for
//     it until the next step's clamp.
//   - every step is ONE full nlplant evaluation (AB_ALL: all 42 live nets).  There is no Overload evaluation, hence no coefficient cache to
//     feed or to read.
//   - throughput shape: 128-row workgroups of two waves; wave w evaluates its half of the nets for BOTH waves' aircraft with the two-set
//     phase statements (mlp_phase_asm_dual_ALL_{0,1}: one weight stream feeds two accumulator sets), the coefficient matrix and the
//     partner's normalised inputs in LDS as in the pair variant of the env kernel.  Euler carries the state's trigonometry and atmosphere
//     power from the end of one step into the next (computed once per state, as the step kernel's cross-step carry does); rk4 evaluates
//     them per stage.
//   - split shape (Euler): eight waves share ONE 64-row tile, each evaluates its slice of PLAN8_ALL; the serial fp64 chains of the state
//     (sines, cosines, tangent, atmosphere power) are computed once per tile and shared through LDS as in the latency family.  For grids
//     that would otherwise leave most CUs idle (np_f16_host.h::rollout_shape).
//   - rows are independent: a plain grid of one workgroup per tile, the ragged tail masked; no workgroup waits for another.
#include "np_model_rollout.h"

#include "np_f16_device.h"
#include "np_f16_kargs.h"

namespace npf16 {

typedef const RolloutArgs __attribute__((address_space(4))) *RolloutArgsC;

// waves per SIMD the register allocator builds for: the Euler throughput shape three (as the pair variant of the step kernel), rk4 two (its
// four stages keep 48 derivatives live on top of the loop's state: built for three it spills, as the rk4 fleet kernels did), the split
// shape two (one eight-wave workgroup per CU is two waves per SIMD)
template <int SOLVER, int SHAPE>
__global__ __launch_bounds__(SHAPE == ROLLOUT_SPLIT ? ROLLOUT_TILE_SPLIT * ROLLOUT_SPLIT_WAVES : ROLLOUT_TILE_THROUGHPUT)
__attribute__((amdgpu_waves_per_eu((SOLVER == 1 || SHAPE == ROLLOUT_SPLIT ? 2 : 3), 8)))
void f16_rollout_kernel(const RolloutArgs a) {
    constexpr bool SPLIT = SHAPE == ROLLOUT_SPLIT;
    static_assert(!SPLIT || SOLVER == 0, "the split shape shares the state's scalars once per step: Euler only");
    constexpr int TILE = SPLIT ? ROLLOUT_TILE_SPLIT : ROLLOUT_TILE_THROUGHPUT;
    constexpr int WPT = SPLIT ? ROLLOUT_SPLIT_WAVES : 2;
    // coefficient columns, then the partner's normalised inputs (throughput) or the tile's shared scalars (split)
    constexpr int COLS = NUM_LDS_SLOTS + (SPLIT ? NUM_SHARED_SCALARS : NUM_NORM_GROUPS);
    __shared__ __attribute__((aligned(16))) float lds[COLS * TILE];
    const int t = SPLIT ? (int)(threadIdx.x % TILE) : (int)threadIdx.x;
    // split: which slice of the nets; throughput: which wave of the pair
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    float *coef = lds + t;  // this lane's coefficient column, stride TILE
    const long long i = (long long)blockIdx.x * TILE + t;
    const bool valid = i < a.rows;
    const unsigned r = (unsigned)(valid ? i : a.rows - 1);  // tail lanes shadow the last row; their stores are masked
    // nothing scalar but `ap` (and the loop's counters) lives across the MLP phases, which own s4-s101: every step re-reads what it needs
    // from the kernel-argument segment (np_f16_device.h, NP_REREAD_ARGS)
    RolloutArgsC ap = (RolloutArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    // rows of every array are (uniform 64-bit base) + (32-bit byte offset): the host keeps ld0, ld_out and rows * act_row_stride below 2^30
    const unsigned src4 = (r / (unsigned)a.fanout) * 4u;
    float s[12], u[4];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = at_off(a.s0 + k * a.ld0, src4);
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = at_off(a.u0 + k * a.ld0, src4);
    const float lef = at_off(a.u0 + 4 * a.ld0, src4);  // the fifth control is not F16Model.update's business: handed through
    const unsigned act4 = r * (unsigned)a.act_row_stride * 4u;
    float act_next[4];
#pragma unroll
    for (int k = 0; k < 4; k++) act_next[k] = at_off(a.actions, act4 + 4u * k);

    StateScalars sc;  // throughput shape, Euler: the trigonometry and atmosphere power of the state at hand, carried from step to step
    if constexpr (!SPLIT && SOLVER == 0) {
        trig_of(s, sc.tr, sc.tt);
        sc.powv = atmos_pow(ap->cfg.af, s[2]);
    }

    int since_record = 0, record = 0;
#pragma nounroll
    for (int step = 0; step < ap->horizon; step++) {
        NP_REREAD_ARGS(ap);
        // ---- F16Model.update (F16_model.py:51-67) ----
        float act[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float v = act_next[k];
            v = v < -1.0f ? -1.0f : v;  // torch.clamp(action, -1, 1); NaN stays NaN
            v = v > 1.0f ? 1.0f : v;
            act[k] = v;
        }
        if (step + 1 < ap->horizon) {  // the next step's action: in flight across this step's net evaluation (a step stride of 0 holds the action)
            const float *nxt = ap->actions + (long long)(step + 1) * ap->act_step_stride;
#pragma unroll
            for (int k = 0; k < 4; k++) act_next[k] = at_off(nxt, act4 + 4u * k);
        }
        control_lag(ap->cfg.af, act, u);
        const AeroWeights wts = {ap->wt.kblob, ap->wt.kblob_dual, ap->wt.pwl, ap->wt.pwl_unnorm, nullptr};
        if constexpr (SOLVER == 0) {  // euler: y1 = y0 + dt*f(y0)
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
        } else {  // torchdiffeq 0.2.3 rk4_alt_step_func (3/8 rule), as the step kernels spell it
            const float dt = ap->cfg.dt;
            const float third = (float)(1.0 / 3.0);
            float y[12], k1[12], k2[12], k3[12];
#pragma unroll
            for (int k = 0; k < 12; k++) y[k] = s[k];
#pragma nounroll
            for (int stage = 0; stage < 4; stage++) {
                float kk[12];
                NP_REREAD_ARGS(ap);
                const AeroWeights wst = {ap->wt.kblob, ap->wt.kblob_dual, ap->wt.pwl, ap->wt.pwl_unnorm, nullptr};
                xdot_full<AB_ALL, TILE, WPT>(wst, airframe_via(ap), y, u, coef, false, kk, pw);
                if (stage == 0) {
#pragma unroll
                    for (int k = 0; k < 12; k++) {
                        k1[k] = kk[k];
                        y[k] = s[k] + (dt * k1[k]) * third;
                    }
                } else if (stage == 1) {
#pragma unroll
                    for (int k = 0; k < 12; k++) {
                        k2[k] = kk[k];
                        y[k] = s[k] + dt * (k2[k] - k1[k] * third);
                    }
                } else if (stage == 2) {
#pragma unroll
                    for (int k = 0; k < 12; k++) {
                        k3[k] = kk[k];
                        y[k] = s[k] + dt * ((k1[k] - k2[k]) + k3[k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 12; k++) y[k] = s[k] + (((k1[k] + 3.0f * (k2[k] + k3[k])) + kk[k]) * dt) * 0.125f;
                }
            }
#pragma unroll
            for (int k = 0; k < 12; k++) s[k] = y[k];
            NP_REREAD_ARGS(ap);
        }
        // ---- the recorded trajectory: the state after steps record_every, 2 * record_every, ... ----
        if (ap->s_traj && ++since_record == ap->record_every) {
            since_record = 0;
            if (valid && (!SPLIT || pw == 0)) {
                float *rec = ap->s_traj + (long long)record * ap->traj_step_stride;
#pragma unroll
                for (int k = 0; k < 12; k++) at_off(rec + k * ap->ld_out, r * 4u) = s[k];
            }
            record++;
        }
    }

    if (valid && (!SPLIT || pw == 0)) {
        NP_REREAD_ARGS(ap);
        const unsigned w4 = r * 4u;
#pragma unroll
        for (int k = 0; k < 12; k++) at_off(ap->s_out + k * ap->ld_out, w4) = s[k];
#pragma unroll
        for (int k = 0; k < 4; k++) at_off(ap->u_out + k * ap->ld_out, w4) = u[k];
        at_off(ap->u_out + 4 * ap->ld_out, w4) = lef;
    }
}

hipError_t launch_model_rollout(int solver, int shape, const RolloutArgs &args, hipStream_t stream) {
    if (solver < 0 || solver > 1 || (shape != ROLLOUT_THROUGHPUT && shape != ROLLOUT_SPLIT) || (solver == 1 && shape == ROLLOUT_SPLIT) || args.rows <= 0)
        return hipErrorInvalidValue;
    const int tile = shape == ROLLOUT_SPLIT ? ROLLOUT_TILE_SPLIT : ROLLOUT_TILE_THROUGHPUT;
    const dim3 grid((unsigned)((args.rows + tile - 1) / tile));
    if (shape == ROLLOUT_SPLIT)
        hipLaunchKernelGGL((f16_rollout_kernel<0, ROLLOUT_SPLIT>), grid, dim3(ROLLOUT_TILE_SPLIT * ROLLOUT_SPLIT_WAVES), 0, stream, args);
    else if (solver == 0)
        hipLaunchKernelGGL((f16_rollout_kernel<0, ROLLOUT_THROUGHPUT>), grid, dim3(ROLLOUT_TILE_THROUGHPUT), 0, stream, args);
    else
        hipLaunchKernelGGL((f16_rollout_kernel<1, ROLLOUT_THROUGHPUT>), grid, dim3(ROLLOUT_TILE_THROUGHPUT), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
