// np_env_launch.h — the hand-over between the host side of np_f16_step / np_f16_reset (np_f16_kernels.hip::launch_env: argument checks,
// dispatch rule np_dispatch.h::env_choice, timing events) and the translation units that hold the instantiations of f16_env_kernel
// (np_env_t{task}s{solver}.hip, np_env_gemm_t{task}s{solver}.hip <- np_env_tu.inc) and of f16_fleet_kernel (np_env_fleet_t{task}s{solver}.hip).
// One unit per task x solver x {plain, GEMM, fleet}: the eighteen compile side by side instead of one after the other.
#pragma once
#include <hip/hip_runtime.h>

#include "np_dispatch.h"
#include "np_f16_kargs.h"

namespace npf16 {

struct EnvLaunch {
    KArgs a;
    npdispatch::EnvChoice ch;  // variant flags, grid and block of this launch
    hipStream_t st;
    bool timed;                // start / stop attached to the dispatch itself (hipExtLaunchKernelGGL)
    hipEvent_t start, stop;
    bool step;                 // np_f16_step (true) or np_f16_reset
    bool inner;                // np_f16_io.inner_step (step only)
    bool cached;               // the cross-step coefficient cache is valid for this launch (step only)
    FleetRef fleet;            // contexts with a fleet (np_f16_set_fleet; k = 0 otherwise): the class table and this launch's rows of the index
};

// TASK = 0 heading, 1 control, 2 tracking; SOLVER = 0 euler, 1 rk4 (3/8 rule); GEMM: contexts with aero_gemm_order (single-set family only).
// Each unit defines its own specialisation; a reset goes to the solver-0 unit of its task.
template <int TASK, int SOLVER, bool GEMM>
void env_dispatch(const EnvLaunch &l);

// Contexts with a fleet: the instantiations of f16_fleet_kernel (np_env_fleet_t{task}s{solver}.hip <- np_env_tu.inc with NP_ENV_FLEET), the
// throughput shape at every n; l.ch carries the grid and the block of that shape.
template <int TASK, int SOLVER>
void env_dispatch_fleet(const EnvLaunch &l);

}  // namespace npf16
