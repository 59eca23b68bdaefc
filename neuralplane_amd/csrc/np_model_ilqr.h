// np_model_ilqr.h — the argument record and the launcher of iLQR's backward pass on the flight model (np_model_ilqr.hip), as
// np_f16_kernels.hip's np_f16_model_ilqr_backward sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_f16_types.h"

namespace npf16 {

// One launch = the Riccati sweep over `horizon` Euler applications of F16Model.update (envs/models/F16_model.py:51-67) for rows = n0 * fanout
// rows, about the states the rollout recorded.  Every array is device memory and planar; strides are in floats.
struct IlqrArgs {
    const float *s0, *u0;        // the start: [12][ld0], [5][ld0]; output row r started from row r / fanout
    long long ld0;
    const float *actions;        // step t, row r: actions + t * act_step_stride + r * act_row_stride, four floats
    long long act_step_stride, act_row_stride;
    const float *s_traj;         // the state after step t + 1: [12][ld_traj] at s_traj + t * traj_step_stride (rollout, record_every = 1)
    const float *g_s_traj;       // d cost / d s_{t+1}, same layout
    long long traj_step_stride;
    const float *g_actions_in;   // the direct d cost / d a_t: [horizon][4][ld_traj]
    const float *g_u_end;        // d cost / d u_H[0:4], [4][ld_traj]; may be null (zero)
    const float *h_s;            // the Gauss-Newton diagonal of the state cost, [horizon][12], shared by the rows
    const float *mu_rows;        // the regularisation per row, [rows]; null = `mu` for every row
    float *k, *K, *dV;           // [horizon][4][ld_out], [horizon][64][ld_out] (entry 16 a + j), [2][ld_out]
    int *status;                 // [rows]: -1, or the step the row stopped at
    float *p0, *P0;              // [16][ld_out], [256][ld_out] (entry 16 i + j); both null or both given
    float *u_ws;                 // workspace: the lagged controls u_1..u_H, [horizon][4][ld_traj]
    float *p_ws;                 // workspace: the value Hessian between steps, [rows][256] in the accumulator's order
    long long ld_traj, ld_out;
    long long rows;              // n0 * fanout
    int horizon, fanout;
    float dt, mu;
    float h_a[4];                // the Gauss-Newton diagonal of the action cost
    const float *kblob;          // the context's single-set weight blob (np_nets.h, KBLOB_FLOATS floats)
    Airframe af;
};

// `groups` workgroups of LIN_TILE * LIN_WAVES threads, each walking the 64-row tiles blockIdx.x, + gridDim.x, ... (np_f16_host.h::
// linearize_groups).  hipSuccess, the launch error, or hipErrorInvalidValue for rows / groups / horizon < 1
hipError_t launch_model_ilqr_backward(int groups, const IlqrArgs &args, hipStream_t stream);

}  // namespace npf16
