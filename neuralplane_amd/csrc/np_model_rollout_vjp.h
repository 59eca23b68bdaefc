// np_model_rollout_vjp.h — the argument record and the launcher of the rollout's reverse sweep (np_model_rollout_vjp.hip), as
// np_f16_kernels.hip's np_f16_model_rollout_vjp sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_f16_types.h"

namespace npf16 {

// One launch = the vector-Jacobian product of `horizon` Euler applications of F16Model.update (envs/models/F16_model.py:51-67) for
// rows = n0 * fanout output rows, about the states the rollout recorded.  Every array is device memory and planar; strides are in floats.
struct RolloutVjpArgs {
    const float *s0, *u0;        // the start: [12][ld0], [5][ld0]; output row r started from row r / fanout
    long long ld0;
    const float *actions;        // step t, row r: actions + t * act_step_stride + r * act_row_stride, four floats (step stride 0 = held)
    long long act_step_stride, act_row_stride;
    const float *s_traj;         // the state after step t + 1: [12][ld_traj] at s_traj + t * traj_step_stride (rollout, record_every = 1)
    const float *g_s_traj;       // its cotangent, same layout
    long long traj_step_stride;
    const float *g_u_end;        // cotangent of the controls after the last step, [5][ld_traj]; may be null (zero)
    float *g_s0, *g_u0;          // [12][ld_out], [5][ld_out]
    float *g_actions;            // laid out as `actions`; four columns written
    float *u_ws;                 // workspace: the lagged controls u_1..u_H, [horizon][4][ld_traj]
    long long ld_traj, ld_out;
    long long rows;              // n0 * fanout
    int horizon, fanout;
    float dt;
    int pad_;
    const float *kblob;          // the context's single-set weight blob (np_nets.h, KBLOB_FLOATS floats)
    Airframe af;
};

// `groups` workgroups of LIN_TILE * LIN_WAVES threads, each walking the 64-row tiles blockIdx.x, + gridDim.x, ... as the linearisation
// kernel does (np_f16_host.h::linearize_groups).  hipSuccess, the launch error, or hipErrorInvalidValue for rows / groups / horizon < 1
hipError_t launch_model_rollout_vjp(int groups, const RolloutVjpArgs &args, hipStream_t stream);

}  // namespace npf16
