// np_model_ekf.h — the argument record and the launcher of the batched extended Kalman filter (np_model_ekf.hip), as np_f16_kernels.hip's
// np_f16_model_ekf sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_f16_types.h"

namespace npf16 {

// One launch = `horizon` predict + update steps of the filter per row (include/neuralplane_amd.h: np_f16_ekf_io).  Every array is device
// memory, strides in floats; everything else is a host value the entry point has prepared in the equilibrated coordinates x = T x~.
struct EkfArgs {
    const float *s0, *u0;        // [12][ld0], [5][ld0]
    long long ld0;
    const float *P0;             // [256][ld], plane 16 i + j
    const float *z;              // [horizon][16][ld]
    long long ld;
    const float *actions;        // step t, row r at actions + t * act_step_stride + r * act_row_stride
    long long act_step_stride, act_row_stride;
    float *s_out, *u_out, *P_out;            // [12][ld_out], [5][ld_out], [256][ld_out]
    int *status;                             // [rows]
    float *x_traj, *pdiag_traj, *nis;        // [horizon][16][ld_out] twice, [horizon][ld_out]; each may be null
    long long ld_out;
    float *p_ws;                 // rows * 256 floats: P~ between steps, in the accumulator's order
    long long rows;
    int horizon, measure;        // bit i of measure: coordinate i of x = (s[12], u[0:4]) has a sensor
    float dt, kappa;             // the context's step and the lag's keep factor
    float q[16];                 // q[i] / t[i]^2
    float nt[16];                // t[i]^2 / r[i] for measured coordinates, 0 elsewhere
    float rinv[16];              // 1 / r[i] for measured coordinates, 0 elsewhere
    float t[16], tinv[16];       // the equilibration: powers of two, tinv = 1 / t exactly
    const float *kblob;          // the context's single-set weight blob
    Airframe af;
};

// `groups` workgroups of LIN_TILE * LIN_WAVES threads (np_f16_host.h::linearize_groups), each walking the 64-row tiles blockIdx.x,
// + gridDim.x, ...  hipSuccess, the launch error, or hipErrorInvalidValue for rows / groups / horizon < 1
hipError_t launch_model_ekf(int groups, const EkfArgs &args, hipStream_t stream);

}  // namespace npf16
