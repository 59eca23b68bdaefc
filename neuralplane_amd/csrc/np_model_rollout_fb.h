// np_model_rollout_fb.h — the feedback rollout kernel's argument record and its launcher (np_model_rollout_fb.hip): iLQR's forward pass,
// as np_f16_kernels.hip's np_f16_model_rollout_feedback sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_model_rollout.h"

namespace npf16 {

// One launch = `horizon` Euler applications of F16Model.update (envs/models/F16_model.py:51-67) under the law
//     a_t = abar_t + alpha k_t + K_t (x_t - xbar_t),   x = (s[12], u[0:4] entering the step)
// to rows = problems * n_alpha output rows: output row r is problem q = r / n_alpha with step size alphas[r % n_alpha], and problem q
// starts from start row q / fanout.  Every array is device memory; strides are in floats; per-problem arrays are planar with pitch ld.
struct FeedbackArgs {
    const float *s0, *u0;        // the nominal start: [12][ld0], [5][ld0]
    long long ld0;
    const float *actions;        // abar: step t, problem q: actions + t * act_step_stride + q * act_row_stride, four floats
    long long act_step_stride, act_row_stride;
    const float *s_traj;         // sbar_{t+1}: [12][ld] at s_traj + t * traj_step_stride (the nominal rollout, record_every = 1)
    long long traj_step_stride;
    const float *k, *K;          // [horizon][4][ld], [horizon][64][ld] (plane 16 a + j = K_t[a][j])
    const float *s_init, *u_init;  // the start the candidates actually fly from: [12][ld], [5][ld]; both null = the nominal start
    const float *s_ref;          // the cost's reference for s_{t+1}: [horizon][12][ld]; read only with `cost`
    const float *ws;             // [FB_WS_ALPHAS] the step sizes, then [horizon][12] the cost's state diagonal
    float *actions_out;          // the clamped actions flown: [horizon][rows][4]
    float *s_out, *u_out;        // [12][ld_out], [5][ld_out]
    float *s_traj_out;           // the state after step t + 1: [12][ld_out] at s_traj_out + t * 12 * ld_out
    float *cost;                 // [rows] or null
    int *best;                   // [problems] or null (n_alpha a power of two)
    long long ld, ld_out;
    long long rows;              // problems * n_alpha
    int horizon, fanout, n_alpha, pad_;
    float h_a[4];
    RolloutCfg cfg;              // `cfg.af` is where the FDM device code looks for the airframe behind an MLP phase
    AeroWeights wt;
};

constexpr int FB_WS_ALPHAS = 64;   // floats of the workspace kept for the step sizes (n_alpha <= 64)

// shape ROLLOUT_THROUGHPUT or ROLLOUT_SPLIT (np_model_rollout.h), as rollout_shape resolves it for `rows`.  hipSuccess, the launch error, or
// hipErrorInvalidValue for a shape that is not built or rows / horizon / n_alpha out of range
hipError_t launch_model_rollout_feedback(int shape, const FeedbackArgs &args, hipStream_t stream);

}  // namespace npf16
