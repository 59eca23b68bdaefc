// np_model_lqr.h — the argument record and the launcher of the batched steady-state LQR (np_model_lqr.hip), as np_f16_kernels.hip's
// np_f16_model_lqr sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace npf16 {

constexpr int LQR_WAVES = 4, LQR_TILE = 16, LQR_MAX_DOUBLINGS = 32;
// status[row]
enum LqrStatus : int { LQR_CONVERGED = 0, LQR_LIMIT = 1, LQR_PIVOT = 3, LQR_NONFINITE = 4 };

// One launch = the discrete algebraic Riccati equation of the `update` step map per row, by structured doubling (include/neuralplane_amd.h:
// np_f16_lqr_io).  A, B, K, P and the per-row outputs are device memory, planar, strides in floats; everything else is a host value the
// entry point has prepared (wave-uniform scalar loads, or one vector load per lane where a lane picks its own coordinate).
struct LqrArgs {
    const float *A, *B;          // [144][ld], [48][ld]: what linearize and trim return
    long long ld;
    float *K, *P;                // [64][ld_out] (entry 16 a + j), [256][ld_out] (entry 16 i + j) or null
    int *doublings, *status;     // [rows]
    float *res;                  // [rows]
    long long ld_out;
    long long rows;
    int select, max_doublings;   // bit i of select: coordinate i of x = (s[12], u[0:4]) takes part
    float tol, dt, kappa;        // the stopping tolerance; the context's step and lag factor
    float gain[4], h_a[4];       // d u'[k] / d a[k] without the clamp; R = diag(h_a)
    float q[16];                 // the equilibrated Q's diagonal: h_s[i] t[i]^2 for selected states, 0 elsewhere
    float t[16], tinv[16];       // the equilibration x = T x~: powers of two, tinv = 1 / t exactly
};

// The workgroups the launch takes for n rows on num_cus CUs: one per tile of LQR_TILE rows, at most max_groups (0 = as many as stay resident)
inline int lqr_groups(long long n, int num_cus, int max_groups) {
    const long long tiles = (n + LQR_TILE - 1) / LQR_TILE;
    const long long cap = max_groups > 0 ? max_groups : 2ll * num_cus;
    return (int)(tiles < cap ? tiles : cap);
}

// `groups` workgroups of 64 * LQR_WAVES threads, each walking the 16-row tiles blockIdx.x, + gridDim.x, ...  hipSuccess, the launch error,
// or hipErrorInvalidValue for rows / groups < 1
hipError_t launch_model_lqr(int groups, const LqrArgs &args, hipStream_t stream);

}  // namespace npf16
