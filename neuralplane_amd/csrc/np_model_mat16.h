// np_model_mat16.h — a 16 x 16 fp32 matrix on ONE wave, in the accumulator layout of v_mfma_f32_16x16x4_f32: lane l = 16 g + c holds
// M[4 g + r][c] in register r.  What np_model_lqr.hip (the doubling) and np_model_ekf.hip (the filter's covariance) share: the product with
// no shuffle, the symmetrisation through the wave's transpose area, the in-register Gauss-Jordan solve and the lane helpers.  Device only.
#pragma once
#include "np_f16_device.h"

namespace npf16 {
namespace mat16 {

constexpr int SYM_STRIDE = 17;   // the transpose area: 16 x SYM_STRIDE floats of LDS per wave

// LDS traffic between the lanes of ONE wave: the DS instructions of a wave execute in order; this keeps the compiler from reordering them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T *glob(T *p) {
    return reinterpret_cast<__attribute__((address_space(1))) T *>(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ float lane_get(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ float from_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_ds_bpermute(lane * 4, __float_as_int(v))); }
__device__ __forceinline__ float pick4(int i, const f32x4 &x) { return i == 0 ? x[0] : i == 1 ? x[1] : i == 2 ? x[2] : x[3]; }
__device__ __forceinline__ bool finite4(const f32x4 &x) { return ((x[0] - x[0]) + (x[1] - x[1])) + ((x[2] - x[2]) + (x[3] - x[3])) == 0.0f; }
__device__ __forceinline__ bool wave_any(bool b) { return __builtin_amdgcn_ballot_w64(b) != 0; }

// X^T Y in the accumulator layout: the k index runs in the accumulator's order, so neither operand is shuffled
__device__ __forceinline__ f32x4 mm(const f32x4 &X, const f32x4 &Y) {
    f32x4 C = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; r++) C = __builtin_amdgcn_mfma_f32_16x16x4f32(X[r], Y[r], C, 0, 0, 0);
    return C;
}

// 1/2 (M + M^T) through the wave's transpose area
__device__ __forceinline__ f32x4 sym_half(const f32x4 &M, float *scr, int g, int c) {
    f32x4 out;
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; r++) scr[(4 * g + r) * SYM_STRIDE + c] = M[r];
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; r++) out[r] = 0.5f * (M[r] + scr[c * SYM_STRIDE + 4 * g + r]);
    wave_sync();
    return out;
}

// Gauss-Jordan with partial pivoting on [W | X | Y], rows left in place: on return row p_k of X, Y holds row k of W^-1 [X | Y] and
// PT[r] = 1 where p_c = 4 g + r, so that mm(PT, X) puts the rows back in order.  The pivot row is a wave-uniform choice: each candidate of
// column k becomes an integer key (the bits of |w| with the last four replaced by 15 - row, so ties go to the lowest row).  A pivot with
// |p| <= 2^-20 max_i |W_ik| (W as it came in) is rejected.  0 = done, 1 = a pivot was rejected, 2 = a pivot was NaN
__device__ __forceinline__ int solve(f32x4 &W, f32x4 &X, f32x4 &Y, f32x4 &PT, int g, int c) {
    float cmax = fmaxf(fmaxf(fabsf(W[0]), fabsf(W[1])), fmaxf(fabsf(W[2]), fabsf(W[3])));
    cmax = fmaxf(cmax, from_lane(cmax, (16 * g + c) ^ 16));
    cmax = fmaxf(cmax, from_lane(cmax, (16 * g + c) ^ 32));   // the largest |W_ic| of the lane's column
    unsigned used = 0;
    PT = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 16; k++) {
        unsigned key = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 4 * g + r;
            const unsigned cand = (__float_as_uint(fabsf(W[r])) & ~15u) | (unsigned)(15 - row);
            key = max(key, ((used >> row) & 1u) ? 0u : cand);
        }
        const unsigned k0 = __builtin_amdgcn_readlane(key, k), k1 = __builtin_amdgcn_readlane(key, 16 + k);
        const unsigned k2 = __builtin_amdgcn_readlane(key, 32 + k), k3 = __builtin_amdgcn_readlane(key, 48 + k);
        const int p = 15 - (int)(max(max(k0, k1), max(k2, k3)) & 15u);   // wave-uniform
        const int gp = p >> 2, rp = p & 3;
        const float piv = lane_get(pick4(rp, W), 16 * gp + k);
        if (!(fabsf(piv) > 0x1p-20f * lane_get(cmax, k))) return piv != piv ? 2 : 1;
        const float rw = from_lane(pick4(rp, W), 16 * gp + c) / piv, rx = from_lane(pick4(rp, X), 16 * gp + c) / piv;
        const float ry = from_lane(pick4(rp, Y), 16 * gp + c) / piv;
        float mult[4];
#pragma unroll
        for (int r = 0; r < 4; r++) mult[r] = from_lane(W[r], 16 * g + k);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool is_p = 4 * g + r == p;
            W[r] = is_p ? rw : fmaf(-mult[r], rw, W[r]);
            X[r] = is_p ? rx : fmaf(-mult[r], rx, X[r]);
            Y[r] = is_p ? ry : fmaf(-mult[r], ry, Y[r]);
            if (c == k) PT[r] = is_p ? 1.0f : 0.0f;
        }
        used |= 1u << p;
    }
    return 0;
}

// Gauss-Jordan with partial pivoting on [W | X] alone, the same pivots: on return row p_k of X holds row k of W^-1 X and
// PT as above (one right-hand side fewer: a third fewer FMAs and two lane moves fewer per pivot)
__device__ __forceinline__ int solve(f32x4 &W, f32x4 &X, f32x4 &PT, int g, int c) {
    float cmax = fmaxf(fmaxf(fabsf(W[0]), fabsf(W[1])), fmaxf(fabsf(W[2]), fabsf(W[3])));
    cmax = fmaxf(cmax, from_lane(cmax, (16 * g + c) ^ 16));
    cmax = fmaxf(cmax, from_lane(cmax, (16 * g + c) ^ 32));   // the largest |W_ic| of the lane's column
    unsigned used = 0;
    PT = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 16; k++) {
        unsigned key = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 4 * g + r;
            const unsigned cand = (__float_as_uint(fabsf(W[r])) & ~15u) | (unsigned)(15 - row);
            key = max(key, ((used >> row) & 1u) ? 0u : cand);
        }
        const unsigned k0 = __builtin_amdgcn_readlane(key, k), k1 = __builtin_amdgcn_readlane(key, 16 + k);
        const unsigned k2 = __builtin_amdgcn_readlane(key, 32 + k), k3 = __builtin_amdgcn_readlane(key, 48 + k);
        const int p = 15 - (int)(max(max(k0, k1), max(k2, k3)) & 15u);   // wave-uniform
        const int gp = p >> 2, rp = p & 3;
        const float piv = lane_get(pick4(rp, W), 16 * gp + k);
        if (!(fabsf(piv) > 0x1p-20f * lane_get(cmax, k))) return piv != piv ? 2 : 1;
        const float rw = from_lane(pick4(rp, W), 16 * gp + c) / piv, rx = from_lane(pick4(rp, X), 16 * gp + c) / piv;
        float mult[4];
#pragma unroll
        for (int r = 0; r < 4; r++) mult[r] = from_lane(W[r], 16 * g + k);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool is_p = 4 * g + r == p;
            W[r] = is_p ? rw : fmaf(-mult[r], rw, W[r]);
            X[r] = is_p ? rx : fmaf(-mult[r], rx, X[r]);
            if (c == k) PT[r] = is_p ? 1.0f : 0.0f;
        }
        used |= 1u << p;
    }
    return 0;
}

}  // namespace mat16
}  // namespace npf16
