// np_env_gemm_t0s0.hip — the instantiations of f16_env_kernel<..., GEMM = true> (np_f16_env_kernel.h: the env kernels with the aero nets in GEMM
// order, numerics option aero_gemm_order) for task 0 (0 heading, 1 control, 2 tracking) and solver 0 (0 euler, 1 rk4).
#define NP_ENV_TASK 0
#define NP_ENV_SOLVER 0
#define NP_ENV_GEMM 1
#include "np_env_tu.inc"
