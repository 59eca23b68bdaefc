// np_env_fleet_t2s1.hip — the instantiations of f16_fleet_kernel (np_f16_env_kernel.h: the env kernels with per-row airframes, np_f16_set_fleet)
// for task 2 (0 heading, 1 control, 2 tracking) and solver 1 (0 euler, 1 rk4).
#define NP_ENV_TASK 2
#define NP_ENV_SOLVER 1
#define NP_ENV_FLEET 1
#include "np_env_tu.inc"
