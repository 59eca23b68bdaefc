// np_model_rollout.h — the open-loop model rollout kernel's argument record and its launcher (np_model_rollout.hip), as
// np_f16_kernels.hip's np_f16_model_rollout sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_f16_types.h"

namespace npf16 {

// what the kernel reads of the scenario: the integrator step and the airframe.  The member of RolloutArgs is called `cfg` and holds `af`
// because that is where the FDM device code looks for the airframe behind an MLP phase (np_f16_device.h::AirframeVia)
struct RolloutCfg {
    float dt;
    int pad_;
    Airframe af;
};

// One launch = `horizon` applications of F16Model.update (envs/models/F16_model.py:51-67) to rows = n0 * fanout output rows; output row r
// starts from input row r / fanout.  Every array is device memory; strides are in floats.
struct RolloutArgs {
    const float *s0, *u0;      // [12][ld0], [5][ld0]
    long long ld0;
    const float *actions;      // step t, row r: actions + t * act_step_stride + r * act_row_stride, four floats
    long long act_step_stride, act_row_stride;
    float *s_out, *u_out;      // [12][ld_out], [5][ld_out]
    long long ld_out;
    float *s_traj;             // record j (the state after step (j + 1) * record_every): [12][ld_out] at s_traj + j * traj_step_stride; may be null
    long long traj_step_stride;
    long long rows;            // n0 * fanout
    int horizon, fanout, record_every, pad_;
    RolloutCfg cfg;
    AeroWeights wt;
};

// shapes as np_f16_rollout_io.shape resolves them (np_f16_host.h::rollout_shape)
constexpr int ROLLOUT_THROUGHPUT = 1, ROLLOUT_SPLIT = 2;
constexpr int ROLLOUT_TILE_THROUGHPUT = 128, ROLLOUT_TILE_SPLIT = 64, ROLLOUT_SPLIT_WAVES = 8;

// solver 0 Euler / 1 rk4; shape ROLLOUT_THROUGHPUT or ROLLOUT_SPLIT (Euler only).  hipSuccess, the launch error, or hipErrorInvalidValue
// for a (solver, shape) that is not built
hipError_t launch_model_rollout(int solver, int shape, const RolloutArgs &args, hipStream_t stream);

}  // namespace npf16
