// np_model_mppi.h — the MPPI step's argument record and its launcher (np_model_mppi.hip): sample, fly, cost, re-weight, as
// np_f16_kernels.hip's np_f16_model_mppi sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_model_rollout.h"

namespace npf16 {

// One call = two launches on one stream.  The first flies `horizon` Euler applications of F16Model.update (envs/models/F16_model.py:51-67)
// for rows = problems * candidates output rows — row r is problem q = r / candidates, candidate r % candidates, and starts from start row q
// — under a_t = clamp(fma(sigma, eps[r][t], abar[q][t])) and leaves one cost per row; the second turns a problem's costs into softmin
// weights and the weighted mean of the actions flown, which it makes again from the counters.  Every array is device memory; strides are
// in floats; per-problem arrays are planar with pitch ld.
struct MppiArgs {
    const float *s0, *u0;        // the start: [12][ld0], [5][ld0] (row 4, lef, is not read)
    long long ld0;
    const float *actions;        // abar: step t, problem q: actions + t * act_step_stride + q * act_row_stride, four floats
    long long act_step_stride, act_row_stride;
    const float *s_ref;          // the cost's reference for s_{t+1}: [horizon][12][ld]
    long long ld;
    const float *ws;             // [horizon][12] the cost's state diagonal
    float *cost;                 // [rows]: written by the first kernel, read by the second
    float *actions_out;          // the clamped actions flown, [horizon][rows][4], or null: then nothing is stored per step
    float *plan_out;             // [horizon][problems][4]
    int *best;                   // [problems] or null
    float *ess;                  // [problems] or null
    long long rows;              // problems * candidates
    unsigned long long seed, call0;
    int horizon, candidates, hold, problems;
    float sigma[4], h_a[4];
    float temperature;
    int pad_;
    RolloutCfg cfg;              // `cfg.af` is where the FDM device code looks for the airframe behind an MLP phase
    AeroWeights wt;
};

constexpr int MPPI_MAX_CANDIDATES = 4096;   // the second kernel keeps a problem's weights per wave in LDS
constexpr int MPPI_UPDATE_WAVES = 2;        // waves per workgroup of the second kernel: 2 x 4096 floats of LDS at the most

// shape ROLLOUT_THROUGHPUT or ROLLOUT_SPLIT (np_model_rollout.h), as rollout_shape resolves it for `rows`.  hipSuccess, the first launch
// error, or hipErrorInvalidValue for a shape that is not built or rows / horizon / candidates / hold out of range
hipError_t launch_model_mppi(int shape, const MppiArgs &args, hipStream_t stream);

}  // namespace npf16
