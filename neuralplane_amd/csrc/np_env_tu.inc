// np_env_tu.inc — body of one env-kernel translation unit: #define NP_ENV_TASK / NP_ENV_SOLVER (and NP_ENV_GEMM 1 for the unit of the
// GEMM-order kernels, numerics option aero_gemm_order; or NP_ENV_FLEET 1 for the unit of the fleet kernels, f16_fleet_kernel), then include this file.
// Every variant of f16_env_kernel<NP_ENV_TASK, NP_ENV_SOLVER, ..., NP_ENV_GEMM> the dispatch rule (np_dispatch.h::env_choice) can pick is
// instantiated here and nowhere else; which one a launch gets is decided by the caller (EnvLaunch::ch), this file only maps flags to template arguments.
#include "np_f16_env_kernel.h"
#include "np_env_launch.h"
#ifndef NP_ENV_GEMM
#define NP_ENV_GEMM 0
#endif

#ifdef NP_ENV_FLEET
// the fleet kernels of this task x solver: step (cached or not, inner step / update-only or not) and, in the Euler unit, reset
namespace npf16 {
namespace {

template <int S, bool STEP, bool I>
void launch_fleet(const EnvLaunch &l) {
    constexpr int T = NP_ENV_TASK;
    const auto k = l.cached ? f16_fleet_kernel<T, S, STEP, STEP, I> : f16_fleet_kernel<T, S, STEP, false, I>;
    FleetKArgs fa;
    static_cast<KArgs &>(fa) = l.a;
    fa.fleet = l.fleet;
    const dim3 grid((unsigned)l.ch.grid), block((unsigned)l.ch.block);
    if (l.timed) hipExtLaunchKernelGGL(k, grid, block, 0, l.st, l.start, l.stop, 0, fa);
    else hipLaunchKernelGGL(k, grid, block, 0, l.st, fa);
}

}  // namespace

template <>
void env_dispatch_fleet<NP_ENV_TASK, NP_ENV_SOLVER>(const EnvLaunch &l) {
    if (l.step) {
        if (l.inner) launch_fleet<NP_ENV_SOLVER, true, true>(l);
        else launch_fleet<NP_ENV_SOLVER, true, false>(l);
    }
#if NP_ENV_SOLVER == 0
    else launch_fleet<0, false, false>(l);
#endif
}

}  // namespace npf16
#else
namespace npf16 {
namespace {

constexpr int LAT_TILE = npdispatch::LAT_TILE;

// one variant: with the coefficient cache (a step only) or without, timed or not
template <int S, bool STEP, int TILE, int WPT, bool I, int PW = 2>
void launch(const EnvLaunch &l) {
    constexpr int T = NP_ENV_TASK;
    constexpr bool G = NP_ENV_GEMM;
    const auto k = l.cached ? f16_env_kernel<T, S, STEP, STEP, TILE, WPT, I, PW, G> : f16_env_kernel<T, S, STEP, false, TILE, WPT, I, PW, G>;
    const dim3 grid((unsigned)l.ch.grid), block((unsigned)l.ch.block);
    if (l.timed) hipExtLaunchKernelGGL(k, grid, block, 0, l.st, l.start, l.stop, 0, l.a);
    else hipLaunchKernelGGL(k, grid, block, 0, l.st, l.a);
}

// STEP: env.step or env.reset; I: one low-level iteration of PlanningEnv.step (the three-wave pair build exists for Euler only: six kernels,
// not twelve; the latency family is Euler-only, rk4 falls through to the pair / throughput variants)
template <bool STEP, bool I>
void dispatch(const EnvLaunch &l) {
    constexpr int S = NP_ENV_SOLVER;
    constexpr bool G = NP_ENV_GEMM;
    const npdispatch::EnvChoice &c = l.ch;
    if constexpr (!G) {   // the GEMM-order bodies are single-set: no pair family (env_choice never sets pair / pair3 for such a context)
        if (c.pair3 && (!I || S == 0)) return launch<S, STEP, BLOCK, 2, (I && S == 0), 3>(l);
        if (c.pair) return launch<S, STEP, BLOCK, 2, I>(l);
    }
    if constexpr (S == 0) {   // the latency family is built for Euler only
        if (c.latency8) return launch<0, STEP, LAT_TILE, 8, I>(l);
        if (c.latency2) return launch<0, STEP, LAT_TILE, WPT_LAT2, I>(l);
        if constexpr (!I) {
            if (c.latency4w) return launch<0, STEP, LAT_TILE, 4, false, 4>(l);
        }
        if (c.latency) return launch<0, STEP, LAT_TILE, 4, I>(l);
    }
    launch<S, STEP, BLOCK, 1, I>(l);
}

}  // namespace

template <>
void env_dispatch<NP_ENV_TASK, NP_ENV_SOLVER, bool(NP_ENV_GEMM)>(const EnvLaunch &l) {
    if (l.step) {
        if (l.inner) dispatch<true, true>(l);
        else dispatch<true, false>(l);
    }
#if NP_ENV_SOLVER == 0   // np_f16_reset has no solver: its kernels live in the Euler unit of the task
    else dispatch<false, false>(l);
#endif
}

}  // namespace npf16
#endif
