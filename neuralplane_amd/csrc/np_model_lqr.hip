// np_model_lqr.hip — steady-state LQR gains at operating points: the discrete algebraic Riccati equation of the `update` step map, per row
// and in ONE launch (np_f16_model_lqr), by the structured doubling algorithm.  No nets are evaluated: the inputs are the A and B that
// linearize / trim return.  With x = (s[12], u[0:4]) (np_model_ilqr.hip's coordinates), M = diag(select) and the step map
//     Phi = [[I + dt A, dt B], [0, I]],  S = diag(1 x 12, kappa x 4),  D = diag(gain_k)   (no clamp: an operating point's actions are interior)
//     A_d = M Phi S M,  B_d = M Phi[:, 12:16] D,  Q = M diag(h_s, 0 x 4) M,  R = diag(h_a)
// taken in the equilibrated coordinates x = T x~ (T diagonal, powers of two from the host: A_d <- T^-1 A_d T, B_d <- T^-1 B_d, Q <- T Q T; every
// scaling is exact), the doubling runs from A = A_d, G = B_d R^-1 B_d^T, H = Q:
//     W = I + G H;  X = W^-1 A;  Y = W^-1 G;  A+ = A X;  G+ = G + sym(A Y A^T);  H+ = H + sym(A^T H X)
// and stops at the first doubling with max_ij |H+_ij - H_ij| / sqrt(H+_ii H+_jj) <= tol (pairs with H+_ii H+_jj > 0), or at max_doublings, or
// before a doubling whose result leaves fp32's range.  Then K = -(R + B_d^T H B_d)^-1 B_d^T H A_d by the square-root-free 4 x 4 LDL^T of
// np_model_ilqr.hip, and K T^-1, T^-1 H T^-1 are the caller's K and P.
//
// Schedule: a WAVE IS A PROBLEM.  A, A^T, G and H sit in the accumulator layout of v_mfma_f32_16x16x4_f32 (lane l = 16 g + c holds M[4 g + r][c]
// in register r), in which mm(X, Y) = sum_r mfma(a = X_r, b = Y_r) is X^T Y with no shuffle.  Carrying A^T beside A, and G, H symmetric, makes
// every product of the recursion such a call: nine per doubling, 36 MFMAs.
//   - the solve W [X | Y] = [A | G]: Gauss-Jordan over 16 pivots on the 16 x 48 matrix in twelve registers per lane, partial pivoting with
//     the rows left in place.  The pivot row is a wave-uniform choice: each candidate of column k becomes an integer key (the bits of |w|
//     with the last four replaced by 15 - row, so ties go to the lowest row), four v_readlane and three scalar maxima pick it.  The pivot row
//     reaches the lanes of its columns by three ds_bpermute, the multipliers the lanes of their rows by four; a lane's update is twelve
//     FMAs.  Row p_k then holds row k of the result: a permutation, applied as two more products with the 0 / 1 matrix the pivots wrote
//     (exact).  A pivot with |p| <= 2^-20 max_i |W_ik| (W as the doubling formed it) is rejected.
//   - sym() transposes through 272 floats of LDS per wave; the criterion's diagonal goes by five ds_bpermute, its maximum by a butterfly.
//   - no workspace: the iterates never leave the registers.  Latency is covered by occupancy (four-wave workgroups, several per CU), not by
//     interleaving problems inside a wave.
//   - a workgroup of four waves walks tiles of 16 consecutive rows: the tile's 192 planes of A and B come in as 64-byte runs per plane into
//     LDS (a row's record: 192 floats, stride 193), wave w solves rows w, w + 4, w + 8, w + 12 of the tile, K and P are staged in LDS
//     (stride 321) and leave as 64-byte runs per plane.  The two barriers per tile are in workgroup-uniform control flow; a row's result
//     does not depend on the tile, the wave or the grid it lands in.
#include "np_model_lqr.h"

#include "np_f16_device.h"
#include "np_model_mat16.h"

namespace npf16 {

constexpr int LQR_IN_PLANES = 192, LQR_IN_STRIDE = 193, LQR_OUT_PLANES = 64 + 256, LQR_OUT_STRIDE = 321, LQR_SYM_STRIDE = mat16::SYM_STRIDE;
constexpr int LQR_LDS_FLOATS = LQR_TILE * (LQR_IN_STRIDE + LQR_OUT_STRIDE) + LQR_WAVES * 16 * LQR_SYM_STRIDE;
static_assert(LQR_LDS_FLOATS * sizeof(float) <= 40 * 1024, "at least two workgroups per CU");
static_assert(LQR_TILE == 4 * LQR_WAVES, "a wave solves four rows of the tile");

typedef const LqrArgs __attribute__((address_space(4))) *LqrArgsC;

namespace lqr {

using namespace mat16;   // the product, the symmetrisation, the solve and the lane helpers (np_model_mat16.h)

// entry (i, j) of the equilibrated A_d = T^-1 M Phi S M T from the row's record `in` (A as [12][12], then B as [12][4])
__device__ __forceinline__ float a_d(const float *in, LqrArgsC ap, int i, int j) {
    float phi = i == j ? 1.0f : 0.0f;
    if (i < 12) phi = phi + ap->dt * in[j < 12 ? i * 12 + j : 144 + i * 4 + (j - 12)];
    const float m = (float)(((ap->select >> i) & (ap->select >> j)) & 1);
    return ((m * (phi * (j < 12 ? 1.0f : ap->kappa))) * ap->t[j]) * ap->tinv[i];
}
// entry (i, k) of the equilibrated B_d = T^-1 M Phi[:, 12:16] D
__device__ __forceinline__ float b_d(const float *in, LqrArgsC ap, int i, int k) {
    float phi = i == 12 + k ? 1.0f : 0.0f;
    if (i < 12) phi = phi + ap->dt * in[144 + i * 4 + k];
    return (((float)((ap->select >> i) & 1) * phi) * ap->gain[k]) * ap->tinv[i];
}

// Qt = L diag(piv) L^T, unit lower L, row by row in this fixed order; x = -Qt^-1 b (np_model_ilqr.hip)
struct Ldl4 {
    float l10, l20, l21, l30, l31, l32, piv[4];
    __device__ __forceinline__ void factor(const float (&q)[4][4]) {
        piv[0] = q[0][0];
        l10 = q[1][0] / piv[0];
        l20 = q[2][0] / piv[0];
        l30 = q[3][0] / piv[0];
        piv[1] = q[1][1] - l10 * (l10 * piv[0]);
        l21 = (q[2][1] - l20 * (l10 * piv[0])) / piv[1];
        l31 = (q[3][1] - l30 * (l10 * piv[0])) / piv[1];
        piv[2] = (q[2][2] - l20 * (l20 * piv[0])) - l21 * (l21 * piv[1]);
        l32 = ((q[3][2] - l30 * (l20 * piv[0])) - l31 * (l21 * piv[1])) / piv[2];
        piv[3] = ((q[3][3] - l30 * (l30 * piv[0])) - l31 * (l31 * piv[1])) - l32 * (l32 * piv[2]);
    }
    __device__ __forceinline__ void solve_neg(const float (&b)[4], float (&x)[4]) const {
        const float y0 = -b[0];
        const float y1 = -b[1] - l10 * y0;
        const float y2 = (-b[2] - l20 * y0) - l21 * y1;
        const float y3 = ((-b[3] - l30 * y0) - l31 * y1) - l32 * y2;
        x[3] = y3 / piv[3];
        x[2] = y2 / piv[2] - l32 * x[3];
        x[1] = (y1 / piv[1] - l21 * x[2]) - l31 * x[3];
        x[0] = ((y0 / piv[0] - l10 * x[1]) - l20 * x[2]) - l30 * x[3];
    }
};

// One problem on one wave: the row's record `in` (LDS) -> its 320 numbers in `out` (LDS: K as [4][16], then P as [16][16]); the row's
// doublings, criterion and status come back in registers (wave-uniform)
__device__ __forceinline__ void problem(const float *in, float *out, float *scr, LqrArgsC ap, int lane, int &doublings_out, float &res_out, int &status_out) {
    const int g = lane >> 4, c = lane & 15;
    f32x4 A, At, G, H;
    float bc[4];   // row c of B_d
#pragma unroll
    for (int k = 0; k < 4; k++) bc[k] = b_d(in, ap, c, k);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = 4 * g + r;
        A[r] = a_d(in, ap, i, c);
        At[r] = a_d(in, ap, c, i);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) s = s + (b_d(in, ap, i, k) * bc[k]) / ap->h_a[k];   // (b_ik b_jk) / h_a[k]: symmetric to the bit
        G[r] = s;
        H[r] = i == c ? ap->q[c] : 0.0f;
    }
    int status = LQR_LIMIT, doublings = 0;
    float res = __builtin_inff();
    if (wave_any(!finite4(A) || !finite4(G))) status = LQR_NONFINITE;

    if (status == LQR_LIMIT) {
#pragma nounroll
        for (int j = 0; j < ap->max_doublings; j++) {
            f32x4 W = mm(G, H), X = A, Y = G, PT;   // G symmetric: G^T H = G H
#pragma unroll
            for (int r = 0; r < 4; r++) W[r] = W[r] + (4 * g + r == c ? 1.0f : 0.0f);
            const int bad = solve(W, X, Y, PT, g, c);
            if (bad) {
                status = bad == 2 ? LQR_LIMIT : LQR_PIVOT;   // a NaN pivot: G H left fp32's range, the recursion diverges
                break;
            }
            X = mm(PT, X);   // the rows back in order
            Y = mm(PT, Y);
            const f32x4 An = mm(At, X), Atn = mm(X, At);            // A X and X^T A^T
            const f32x4 HX = mm(H, X), AHX = mm(A, HX);             // H X (H symmetric) and A^T (H X)
            const f32x4 Z = mm(Y, At), AYA = mm(Z, At);             // Y^T A^T and its transpose times A^T = A Y A^T
            const f32x4 sh = sym_half(AHX, scr, g, c), sg = sym_half(AYA, scr, g, c);
            f32x4 Hn, Gn;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                Hn[r] = H[r] + sh[r];
                Gn[r] = G[r] + sg[r];
            }
            if (wave_any(!finite4(An) || !finite4(Atn) || !finite4(Gn) || !finite4(Hn))) break;   // the doubling is not taken: status 1 with the last H
            // the criterion: H+'s diagonal for the lane's column and for its four rows
            const float dc = from_lane(pick4(c & 3, Hn), 16 * (c >> 2) + c);
            float crit = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float dd = dc * from_lane(Hn[r], 20 * g + r);
                crit = fmaxf(crit, dd > 0.0f ? fabsf(Hn[r] - H[r]) / sqrtf(dd) : 0.0f);
            }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) crit = fmaxf(crit, from_lane(crit, lane ^ m));
            A = An; At = Atn; G = Gn; H = Hn;
            doublings = j + 1;
            res = lane_get(crit, 0);
            if (res <= ap->tol) {
                status = LQR_CONVERGED;
                break;
            }
        }
    }

    // ---- the gain of H: E = B_d^T H A_d and Qt = R + B_d^T H B_d on MFMA; lane c of group 0 holds column c of E in its four registers ----
    float Kc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (status == LQR_CONVERGED || status == LQR_LIMIT) {
        f32x4 A0, Bp;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            A0[r] = a_d(in, ap, 4 * g + r, c);
            const float b = b_d(in, ap, 4 * g + r, c & 3);
            Bp[r] = c < 4 ? b : 0.0f;   // B_d padded to 16 columns
        }
        const f32x4 E = mm(Bp, mm(H, A0)), BHB = mm(Bp, mm(H, Bp));
        float q[4][4], e[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            e[k] = E[k];
#pragma unroll
            for (int j2 = 0; j2 <= k; j2++) {   // the lower triangle, mirrored
                q[k][j2] = lane_get(BHB[k], j2) + (j2 == k ? ap->h_a[k] : 0.0f);
                q[j2][k] = q[k][j2];
            }
        }
        Ldl4 f;
        f.factor(q);
        const float inf = __builtin_inff();
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 4; k++) bad = bad || !(f.piv[k] > 0.0f) || !(f.piv[k] < inf);
        if (bad) status = LQR_PIVOT;   // wave-uniform: q is
        else f.solve_neg(e, Kc);
    }
    const float fill = status == LQR_NONFINITE ? __builtin_nanf("") : 0.0f;
    const bool plain = status == LQR_CONVERGED || status == LQR_LIMIT;
    const float tc = ap->tinv[c];
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) out[16 * k + c] = plain ? Kc[k] * tc : fill;   // K = K~ T^-1
    }
#pragma unroll
    for (int r = 0; r < 4; r++) out[64 + 16 * (4 * g + r) + c] = plain ? (H[r] * ap->tinv[4 * g + r]) * tc : fill;   // P = T^-1 H T^-1
    doublings_out = doublings;
    res_out = status == LQR_NONFINITE ? fill : res;
    status_out = status;
}

}  // namespace lqr

// built for two waves per SIMD (196 VGPRs unforced, no scratch): two four-wave workgroups per CU
__global__ __launch_bounds__(64 * LQR_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_lqr_kernel(const LqrArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LQR_LDS_FLOATS];
    float *in = lds, *out = lds + LQR_TILE * LQR_IN_STRIDE;
    const int lane = (int)(threadIdx.x & 63);
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *scr = out + LQR_TILE * LQR_OUT_STRIDE + pw * 16 * LQR_SYM_STRIDE;
    LqrArgsC ap = (LqrArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    const long long tiles = (a.rows + LQR_TILE - 1) / LQR_TILE;
#pragma nounroll
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long base = tile * LQR_TILE;
        // ---- the tile's A and B: 16 rows of a plane are one 64-byte run (tail rows shadow the last row; nobody solves them) ----
#pragma unroll 4
        for (int idx = (int)threadIdx.x; idx < LQR_IN_PLANES * LQR_TILE; idx += 64 * LQR_WAVES) {
            const int plane = idx >> 4, pr = idx & 15;
            const long long row = base + pr < ap->rows ? base + pr : ap->rows - 1;
            const float v = plane < 144 ? lqr::glob(ap->A)[(long long)plane * ap->ld + row] : lqr::glob(ap->B)[(long long)(plane - 144) * ap->ld + row];
            in[pr * LQR_IN_STRIDE + plane] = v;
        }
        __syncthreads();   // the records are complete; the previous tile's results have left the staging area

#pragma nounroll
        for (int jj = 0; jj < LQR_TILE / LQR_WAVES; jj++) {
            const int pr = pw + LQR_WAVES * jj;
            const long long row = base + pr;
            if (row < ap->rows) {   // wave-uniform
                int doublings, status;
                float res;
                lqr::problem(in + pr * LQR_IN_STRIDE, out + pr * LQR_OUT_STRIDE, scr, ap, lane, doublings, res, status);
                if (lane == 0) {
                    lqr::glob(ap->doublings)[row] = doublings;
                    lqr::glob(ap->res)[row] = res;
                    lqr::glob(ap->status)[row] = status;
                }
            }
        }
        __syncthreads();   // the tile's K and P are staged; every wave is through with the records

        const int planes = ap->P ? LQR_OUT_PLANES : 64;
#pragma unroll 4
        for (int idx = (int)threadIdx.x; idx < planes * LQR_TILE; idx += 64 * LQR_WAVES) {
            const int plane = idx >> 4, pr = idx & 15;
            if (base + pr < ap->rows) {
                const float v = out[pr * LQR_OUT_STRIDE + plane];
                if (plane < 64) lqr::glob(ap->K)[(long long)plane * ap->ld_out + base + pr] = v;
                else lqr::glob(ap->P)[(long long)(plane - 64) * ap->ld_out + base + pr] = v;
            }
        }
    }
}

hipError_t launch_model_lqr(int groups, const LqrArgs &args, hipStream_t stream) {
    if (groups < 1 || args.rows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_lqr_kernel, dim3((unsigned)groups), dim3(64 * LQR_WAVES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
