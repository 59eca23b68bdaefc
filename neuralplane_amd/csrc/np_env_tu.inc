// np_env_tu.inc — body of one env-kernel translation unit: #define NP_ENV_TASK / NP_ENV_SOLVER (and NP_ENV_GEMM for the unit of the
// GEMM-order kernels, numerics option aero_gemm_order), then include this file.
// Every variant of f16_env_kernel<NP_ENV_TASK, NP_ENV_SOLVER, ...> the dispatch rule (np_dispatch.h::env_choice) can pick is instantiated
// here and nowhere else; which one a launch gets is decided by the caller (EnvLaunch's flags), this file only maps flags to template arguments.
#include "np_f16_env_kernel.h"
#ifdef NP_ENV_GEMM   // second pass over the kernel's text: f16_env_kernel_gemm (see the head of np_f16_env_kernel.h)
#undef NP_ENV_KERNEL_NAME
#undef NP_ENV_KERNEL_GEMM
#define NP_ENV_KERNEL_NAME f16_env_kernel_gemm
#define NP_ENV_KERNEL_GEMM true
#include "np_f16_env_kernel.h"
#endif
#include "np_env_launch.h"
#include "np_dispatch.h"

namespace npf16 {
namespace {

constexpr int LAT_TILE = npdispatch::LAT_TILE;

#define NP_DISPATCH(...)                                                                                                              \
    do {                                                                                                                              \
        if (l.timed) hipExtLaunchKernelGGL((__VA_ARGS__), dim3(l.grid), dim3(l.block), 0, l.st, l.start, l.stop, 0, l.a);             \
        else hipLaunchKernelGGL((__VA_ARGS__), dim3(l.grid), dim3(l.block), 0, l.st, l.a);                                            \
    } while (0)

// STEP: env.step or env.reset; I: one low-level iteration of PlanningEnv.step (the three-wave pair build exists for Euler only: six kernels,
// not twelve; the latency family is Euler-only, rk4 falls through to the pair / throughput variants)
#ifdef NP_ENV_GEMM   // the unit of the GEMM-order kernels (contexts with aero_gemm_order): the single-set family only — the caller never sets pair / pair3
template <bool STEP, bool I>
void dispatch(const EnvLaunch &l) {
    constexpr int T = NP_ENV_TASK, S = NP_ENV_SOLVER;
    const bool cached = l.cached;
    if constexpr (S == 0) {
        if (l.latency8) {
            if (cached) NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, STEP, LAT_TILE, 8, I>);
            else NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, false, LAT_TILE, 8, I>);
            return;
        }
        if (l.latency2) {
            if (cached) NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, STEP, LAT_TILE, WPT_LAT2, I>);
            else NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, false, LAT_TILE, WPT_LAT2, I>);
            return;
        }
        if constexpr (!I) {
            if (l.latency4w) {
                if (cached) NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, STEP, LAT_TILE, 4, false, 4>);
                else NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, false, LAT_TILE, 4, false, 4>);
                return;
            }
        }
        if (l.latency) {
            if (cached) NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, STEP, LAT_TILE, 4, I>);
            else NP_DISPATCH(f16_env_kernel_gemm<T, 0, STEP, false, LAT_TILE, 4, I>);
            return;
        }
    }
    if (cached) NP_DISPATCH(f16_env_kernel_gemm<T, S, STEP, STEP, BLOCK, 1, I>);
    else NP_DISPATCH(f16_env_kernel_gemm<T, S, STEP, false, BLOCK, 1, I>);
}
#else
template <bool STEP, bool I>
void dispatch(const EnvLaunch &l) {
    constexpr int T = NP_ENV_TASK, S = NP_ENV_SOLVER;
    const bool cached = l.cached;
    if (l.pair3 && (!I || S == 0)) {
        if (cached) NP_DISPATCH(f16_env_kernel<T, S, STEP, STEP, BLOCK, 2, (I && S == 0), 3>);
        else NP_DISPATCH(f16_env_kernel<T, S, STEP, false, BLOCK, 2, (I && S == 0), 3>);
        return;
    }
    if (l.pair) {
        if (cached) NP_DISPATCH(f16_env_kernel<T, S, STEP, STEP, BLOCK, 2, I>);
        else NP_DISPATCH(f16_env_kernel<T, S, STEP, false, BLOCK, 2, I>);
        return;
    }
    if constexpr (S == 0) {   // the latency family is built for Euler only
        if (l.latency8) {
            if (cached) NP_DISPATCH(f16_env_kernel<T, 0, STEP, STEP, LAT_TILE, 8, I>);
            else NP_DISPATCH(f16_env_kernel<T, 0, STEP, false, LAT_TILE, 8, I>);
            return;
        }
        if (l.latency2) {
            if (cached) NP_DISPATCH(f16_env_kernel<T, 0, STEP, STEP, LAT_TILE, WPT_LAT2, I>);
            else NP_DISPATCH(f16_env_kernel<T, 0, STEP, false, LAT_TILE, WPT_LAT2, I>);
            return;
        }
        if constexpr (!I) {
            if (l.latency4w) {
                if (cached) NP_DISPATCH(f16_env_kernel<T, 0, STEP, STEP, LAT_TILE, 4, false, 4>);
                else NP_DISPATCH(f16_env_kernel<T, 0, STEP, false, LAT_TILE, 4, false, 4>);
                return;
            }
        }
        if (l.latency) {
            if (cached) NP_DISPATCH(f16_env_kernel<T, 0, STEP, STEP, LAT_TILE, 4, I>);
            else NP_DISPATCH(f16_env_kernel<T, 0, STEP, false, LAT_TILE, 4, I>);
            return;
        }
    }
    if (cached) NP_DISPATCH(f16_env_kernel<T, S, STEP, STEP, BLOCK, 1, I>);
    else NP_DISPATCH(f16_env_kernel<T, S, STEP, false, BLOCK, 1, I>);
}
#endif
#undef NP_DISPATCH

}  // namespace

#define NP_ENV_CAT2(a, b, c, d) a##b##c##d
#define NP_ENV_CAT(a, b, c, d) NP_ENV_CAT2(a, b, c, d)
#ifdef NP_ENV_GEMM
void NP_ENV_CAT(env_dispatch_gemm_t, NP_ENV_TASK, s, NP_ENV_SOLVER)(const EnvLaunch &l) {
#else
void NP_ENV_CAT(env_dispatch_t, NP_ENV_TASK, s, NP_ENV_SOLVER)(const EnvLaunch &l) {
#endif
    if (l.step) {
        if (l.inner) dispatch<true, true>(l);
        else dispatch<true, false>(l);
    }
#if NP_ENV_SOLVER == 0   // np_f16_reset has no solver: its kernels live in the Euler unit of the task
    else dispatch<false, false>(l);
#endif
}

}  // namespace npf16
