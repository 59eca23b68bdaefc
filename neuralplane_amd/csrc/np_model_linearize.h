// np_model_linearize.h — the linearisation kernel's argument record and its launcher (np_model_linearize.hip), as np_f16_kernels.hip's
// np_f16_model_linearize sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_f16_types.h"

namespace npf16 {

// One launch = xdot = f(s, u), A = df/ds [12][12] and B = df/du [12][4] of F16Dynamics.nlplant (envs/models/F16/F16_dynamics.py:37-228) for
// `rows` rows.  Every array is device memory and planar; strides are in floats.
struct LinearizeArgs {
    const float *s0, *u0;   // [12][ld0], [5][ld0]
    long long ld0;
    float *xdot;            // [12][ld_out]; may be null
    float *A, *B;           // plane i * 12 + j of A = df_i/ds_j, plane i * 4 + j of B = df_i/du_j; [144][ld_out], [48][ld_out]
    long long ld_out;
    long long rows;
    const float *kblob;     // the context's single-set weight blob (np_nets.h, KBLOB_FLOATS floats)
    Airframe af;
};

constexpr int LIN_TILE = 64, LIN_WAVES = 8;
// workgroups per CU of the largest grid (np_f16_host.h::linearize_groups): a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
// on ONE copy of the weight blob.  One, because one workgroup's LDS (88 KB) is all that fits a CU: a larger grid would only queue workgroups
// that copy the blob again
constexpr int LIN_GROUPS_PER_CU = 1;

// `groups` workgroups of LIN_TILE * LIN_WAVES threads; hipSuccess, the launch error, or hipErrorInvalidValue for rows / groups < 1
hipError_t launch_model_linearize(int groups, const LinearizeArgs &args, hipStream_t stream);

}  // namespace npf16
