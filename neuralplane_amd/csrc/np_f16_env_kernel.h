// np_f16_env_kernel.h — the fused F-16 env.step / env.reset kernel template (reference: envs/env_base.py:83-109), shared by the
// translation units that instantiate it: np_env_t{0,1,2}s{0,1}.hip and np_env_gemm_t{0,1,2}s{0,1}.hip (one per task x solver x GEMM, built in
// parallel; np_env_tu.inc; the body itself is np_f16_env_body.inc, shared with f16_fleet_kernel at the end of this file) — the host side (context, dispatch rule, C ABI) is np_f16_kernels.hip, which hands a launch over through
// np_env_launch.h.  The numerics option aero_gemm_order (the aero nets in GEMM order) is the kernel's last template parameter, GEMM: a
// compile-time constant of the instantiation, never a run-time branch; the np_env_gemm_* units instantiate the single-set family with it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>

#include "../../include/neuralplane_amd.h"
#include "np_f16_device.h"
#include "np_f16_kargs.h"

namespace npf16 {

#ifndef NPF16_BLOCK
#define NPF16_BLOCK 128
#endif
// pair variant, de-phasing of the first generation: (blockIdx % groups) x stagger cycles; groups odd (co-resident workgroups differ
// by powers of two in index).  Two builds of the step kernel: PW = 2 waves per SIMD (an occupancy cap) and PW = 3; since round 3 both
// Euler builds need 159 VGPRs and no scratch (rk4: 184 / 0 B and 168 / 64 B per lane) — the numbers of the library at hand are printed by
// tools/code_object_table.py from the code object itself (DESIGN.md carries that table); launch_env picks per grid size.
#ifndef NPF16_PAIR_STAGGER
#define NPF16_PAIR_STAGGER 14000  // PW = 2
#endif
#ifndef NPF16_PAIR_GROUPS
#define NPF16_PAIR_GROUPS 3       // PW = 2
#endif
#ifndef NPF16_PAIR3_STAGGER
#define NPF16_PAIR3_STAGGER 7000  // PW = 3 (round 2: 7 x 9 000, profiles/r02b_ab_sessions.md s25; re-tuned on the round-3 kernel, profiles/r03b_ab_dephasing.log: 9 x 7 000 -1.1 % at N = 1e6, -0.7 % at 1e7)
#endif
#ifndef NPF16_PAIR3_GROUPS
#define NPF16_PAIR3_GROUPS 9      // PW = 3
#endif
#ifndef NPF16_MINWAVES
#define NPF16_MINWAVES 3  // waves per SIMD the register allocator must leave room for
#endif
#ifndef NPF16_STAGGER_CYCLES
#define NPF16_STAGGER_CYCLES 20000  // ~10 us at 2 GHz per phase step; 0 disables the de-phasing
#endif
#ifndef NPF16_ONEGEN_DELAY
#define NPF16_ONEGEN_DELAY 16000  // cycles; 0 disables (see f16_env_kernel)
#endif
#ifndef NPF16_STAGGER_MIN_GENS
#define NPF16_STAGGER_MIN_GENS 2  // de-phase only grids of at least this many generations (experiments: 0 = every grid)
#endif
#ifndef NPF16_STAGGER_CYCLES_LONG
#define NPF16_STAGGER_CYCLES_LONG 30000  // grids of 8 generations and more (N >= 1.6e6 on 256 CUs), see the kernel
#endif

// STEP=true : BaseEnv.step  (env_base.py:99-109)
// STEP=false: BaseEnv.reset (env_base.py:83-97)
// CACHED    : a.cache holds, for every row, the 14 force-side alpha/beta-only coefficients of its CURRENT
//             state (written by the previous step's Overload evaluation) -> the integrator skips them.
// TILE, WPT : aircraft per workgroup and how its waves cooperate.  Results are bit-identical between the variants.
//             WPT = 1, TILE = 128  throughput variant: two independent waves (rk4 fallbacks, the 1-D table mode).
//             WPT = 2, TILE = 128  pair variant (default for large batches): each wave owns 64 aircraft, but the two waves split
//                                  the NETS of every evaluation and evaluate their half for both waves' aircraft (dual asm
//                                  bodies, eval_nets in np_f16_device.h); inputs and coefficients cross through LDS.
//             WPT = 4, TILE = 64   latency variant (small batches): four waves hold the SAME 64 aircraft, split the net
//                                  evaluations and redo the cheap non-MLP arithmetic redundantly, so a step takes ~1/2 of a
//                                  lone wave's time; wave 0 stores.
// INNER     : one low-level iteration of PlanningEnv.step (np_f16_io.inner_step): no auto-reset, flagged rows keep their state, flags
//             accumulate.  A template parameter so that the plain env.step carries none of its selects (~30 VALU instructions).
// GEMM      : numerics option aero_gemm_order (np_f16_device.h::eval_class); single-set bodies only, so never with WPT = 2.
template <int TASK, int SOLVER, bool STEP, bool CACHED, int TILE = BLOCK, int WPT = 1, bool INNER = false, int PW = 2, bool GEMM = false>
// waves per SIMD the register allocator builds for: pair variant PW (PW = 2 is also an occupancy CAP — 159 VGPRs would fit three — for the
// grid sizes where six workgroups per CU are placed unevenly), latency4w four, everything else NPF16_MINWAVES
__global__ __launch_bounds__(TILE * lat_waves(WPT))
__attribute__((amdgpu_waves_per_eu((WPT == 2 ? PW : (WPT == 4 && PW == 4) ? 4 : NPF16_MINWAVES), (WPT == 2 && PW == 2 ? 2 : 8))))
void f16_env_kernel(const KArgs a) {
// The four macros of np_f16_env_body.inc.  They are expanded INSIDE the body and name two of its locals: `ap` (the NP_ENV_KARGS_PTR the body
// makes from the kernel-argument segment; NP_REREAD_ARGS refreshes it) and, in the fleet kernel, `r32` (the lane's row, clamped to n - 1,
// defined before the first use of any of them).  Renaming either in the body means renaming it here and in f16_fleet_kernel below.
#define NP_ENV_KARGS_PTR KArgsC
#define NP_ENV_AF_VIA airframe_via(ap)
#define NP_ENV_AF_HERE ap->cfg.af
#define NP_ENV_OBSERVE(T, ...) observe<T>(ap->cfg, __VA_ARGS__)
#include "np_f16_env_body.inc"
#undef NP_ENV_KARGS_PTR
#undef NP_ENV_AF_VIA
#undef NP_ENV_AF_HERE
#undef NP_ENV_OBSERVE
}

// The fleet kernels (np_f16_set_fleet): row i flies the airframe record table[index[i]] instead of a.cfg.af.  The single-set throughput
// shape only (128-row tile, one aircraft per lane, two independent waves); np_env_fleet_t*s*.hip instantiate them through np_env_tu.inc.
// Every lane loads its record with vector loads (np_f16_device.h::fleet_airframe) where the one-airframe kernels re-read the constants with
// scalar loads: behind the MLP phases, so that no constant lives across the asm statements; `r32` is the lane's row, which the body keeps
// anyway.  Euler: built for NPF16_MINWAVES waves per SIMD like the throughput variant (155-160 VGPRs, no scratch).  rk4: the per-lane constants
// on top of the four stages' 48 live derivatives do not fit 168 registers (52-84 bytes of scratch per lane when built for three waves), so
// the rk4 fleet kernels are built for TWO waves per SIMD and keep everything in registers.  A kernel name of its own: f16_env_kernel's set
// of instantiations is a closed family (tests/test_host_logic_cpu.py).
template <int TASK, int SOLVER, bool STEP, bool CACHED, bool INNER>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu((SOLVER == 1 ? 2 : NPF16_MINWAVES), 8)))
void f16_fleet_kernel(const FleetKArgs a) {
    constexpr int TILE = BLOCK, WPT = 1, PW = 2;
    constexpr bool GEMM = false;
// (`ap` and `r32` are the body's locals: see the note at f16_env_kernel's macros)
#define NP_ENV_KARGS_PTR FleetKArgsC
#define NP_ENV_AF_VIA (FleetVia<FleetKArgsC>{ap, r32})
#define NP_ENV_AF_HERE fleet_airframe_of(ap, r32)
#define NP_ENV_OBSERVE(T, ...) observe<T>(FleetObsCfg{ap->cfg.airspeed, fleet_airframe_of(ap, r32)}, __VA_ARGS__)
#include "np_f16_env_body.inc"
#undef NP_ENV_KARGS_PTR
#undef NP_ENV_AF_VIA
#undef NP_ENV_AF_HERE
#undef NP_ENV_OBSERVE
}

}  // namespace npf16
