// np_model_trim.h — the trim kernel's argument record and its launcher (np_model_trim.hip), as np_f16_kernels.hip's np_f16_model_trim sees them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np_f16_types.h"

namespace npf16 {

constexpr int TRIM_MAX_M = 12, TRIM_Z = 16, TRIM_MAX_ITERS = 64, TRIM_BT_STEPS = 8;
// status[row]
enum TrimStatus : int { TRIM_CONVERGED = 0, TRIM_ITER_LIMIT = 1, TRIM_STALLED = 2, TRIM_SINGULAR = 3, TRIM_NONFINITE = 4, TRIM_RUNNING = -1 };

// One launch = a damped Newton solve per row for z = (s[0..11], u[0..3]): r = (xdot(z) - tgt)[rows] -> 0 over the unknowns q, z = z0 + D q.
// Every array is device memory and planar, strides in floats; D, rows, scale, lo and hi travel in this record (wave-uniform scalar loads).
struct TrimArgs {
    const float *s0, *u0;   // [12][ld0], [5][ld0]: the start
    const float *tgt;       // [12][ld0] or null (zero): the prescribed xdot
    long long ld0;
    float *s, *u;           // [12][ld_out], [5][ld_out]: the returned point (row 4 of u is u0's, handed through)
    float *res;             // [rows]: sqrt(phi) at the returned point
    int *iters, *status;    // [rows]
    int *backtracks;        // [rows] or null: the full steps of the row the Armijo test refused
    float *xdot, *A, *B;    // at the returned point, np_model_linearize.h's layout; A and B come together; all three null = no closing pass
    long long ld_out;
    long long rows;
    const float *kblob;
    int m, max_iters;
    float tol2, pad_;       // tol * tol
    float D[TRIM_Z][TRIM_MAX_M];   // unknown j moves z along column j (columns m.. are zero)
    int row_of[TRIM_MAX_M];        // residual i is row row_of[i] of xdot
    int slot_of[12];               // row k of xdot is residual slot_of[k], or -1
    float scale[12], lo[TRIM_Z], hi[TRIM_Z];
    Airframe af;
};

// `groups` workgroups of LIN_TILE * LIN_WAVES threads (np_model_linearize.h); hipSuccess, the launch error, or hipErrorInvalidValue
hipError_t launch_model_trim(int groups, const TrimArgs &args, hipStream_t stream);

}  // namespace npf16
