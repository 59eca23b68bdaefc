// np_model_ilqr.hip — iLQR's backward pass on the flight model: the Riccati sweep over H Euler applications of F16Model.update (reference
// envs/models/F16_model.py:51-67), per row and in ONE launch (np_f16_model_ilqr_backward).  One model step is
//     u' = kappa u + gain_k clamp(a, -1, 1)      (np_f16_device.h::control_lag; kappa = lag_keep)
//     s' = s + dt f(s, u')                       (nlplant)
// and with x = (s[12], u[0:4]) its Jacobian in (s, u') coordinates is Phi = [[I + dt A, dt B], [0, I]], about (s_t, u_{t+1}) as the rollout
// recorded them (np_model_rollout_vjp.hip: nothing is integrated again).  With D = diag(gain_k 1[-1 <= a_k <= 1]), S = diag(1 x 12, kappa x 4),
// the cost gradients g_s_traj / g_actions_in / g_u_end and the Gauss-Newton diagonals h_s[t] / h_a, the sweep runs t = H-1 .. 0 from
// p = (0, g_u_end), P = 0:
//     p_s += g_s_traj[t];  P_ss += diag(h_s[t])
//     w = Phi^T p;  W = Phi^T P Phi
//     Q_x = S w;  Q_a = D w_u + g_actions_in[t];  Q_xx = S W S;  Q_ax = D W_u: S;  Q_aa = D W_uu D + diag(h_a);  Qt = Q_aa + mu I
//     Qt = L diag(piv) L^T (square-root free: a clamped row's gain is -g / (h_a + mu) to the last bit)
//     k = -Qt^-1 Q_a;  K = -Qt^-1 Q_ax;  dV += (k^T Q_a, 1/2 k^T Q_aa k)
//     p <- Q_x + K^T (Q_aa k + Q_a) + Q_ax^T k;  P <- sym(Q_xx + K^T (Q_aa K + Q_ax) + Q_ax^T K)
// A row STOPS at step t (status[row] = t; its k, K of steps t .. 0 and its dV, p0, P0 are 0) when a pivot is <= 0 or not finite, or when Q_a
// is not finite (a non-finite cost gradient: the pivots do not see p).  A row whose alpha, beta or el is not finite at step t, or with a
// NaN action there, is POISONED as in the linearisation: k, K of steps t .. 0, dV, p0 and P0 are NaN.  Neighbours are untouched either way.
//
// Schedule: the reverse sweep's persistent tile (np_model_rollout_vjp.hip: 64 rows, eight waves, blob in LDS, forward lag pre-pass into u_ws,
// phase 1 = np_model_jets.h::lin_phase1) with the contraction replaced and a third phase added.
//   - phase 2: each wave pushes its two directions through nlplant_jets<2> and STORES its two columns of dt [A | B] into the row's Phi record
//     in LDS (12 x 16 floats per row, stride 193: a lane is a row, odd strides keep the stores conflict-free), and adds g_s_traj[t] to its
//     entries of p (coalesced loads, a lane is a row).  The npos / epos columns are wave 7's.  One barrier.
//   - phase 3: a WAVE IS A 16 x 16 MATRIX.  Wave w takes the rows 8 w .. 8 w + 7 of the tile one at a time.  P sits in the accumulator layout
//     of v_mfma_f32_16x16x4_f32: lane l = 16 g + c holds P[4 g + r][c], r = 0..3.  With phi_r = Phi[4 g + r][c] (four LDS reads per lane),
//         Y = P Phi      = sum_r mfma(a = P_r,   b = phi_r)      (P symmetric: a lane's own P[4 g + r][c] is the A operand P[c][4 g + r])
//         W = Phi^T Y    = sum_r mfma(a = phi_r, b = Y_r)        (the k index runs in the accumulator's order: Y needs no shuffle)
//     eight MFMAs.  S and D are per-lane multiplies.  W's control rows (lanes 48..63) reach every lane of their column by ds_bpermute, Qt's
//     sixteen numbers (lanes 60..63) every lane by v_readlane; every lane factors Qt and solves its own column of K redundantly, and the
//     two rank-4 corrections of P are two more MFMAs (K = 4), the lane of group g supplying entry g of its column.  The transpose for
//     sym() goes through 272 floats of LDS per wave.  w and p are a 17th column on the vector pipe (p: 21 floats per row in LDS, with dV, the
//     stop step and the poison flag).
//   - P between steps: the caller's workspace p_ws [rows][256], in the accumulator's order — four coalesced 256-byte accesses per row, read
//     and written once per row and step by the owning wave (32 more VGPRs live across phases 1 and 2 do not fit; 64 KB of P do not fit
//     beside the blob, the columns and 48 KB of Phi).
//   - k and K are planar ([.][ld]): a wave stages its eight rows' 68 numbers in LDS and writes 32-byte runs per plane.
//   - phase 3's LDS (transpose, staging) is the columns' region, dead between phase 2 and the next phase 1: a third barrier per step.
#include "np_model_ilqr.h"

#include "np_model_jets.h"

namespace npf16 {

// Measurement builds only (tools/microbench/ilqr_cost.py, the phase split): -DNPF16_ILQR_ONLY_PHASE=12 leaves phase 3 out (the results are
// wrong).  0, the default, is the kernel.
#ifndef NPF16_ILQR_ONLY_PHASE
#define NPF16_ILQR_ONLY_PHASE 0
#endif

constexpr int PHI_STRIDE = 12 * 16 + 1;     // a row's Phi record: dt [A | B] as [12][16], padded to an odd stride
constexpr int PV_STRIDE = 21;               // a row's vector state: p[16], dV[2], the stop step (int bits, -1 = running), the poison flag
constexpr int PV_DV = 16, PV_STOP = 18, PV_POISON = 19;
constexpr int SYM_STRIDE = 17, STAGE_PLANES = 64 + 4, STAGE_STRIDE = 9;
constexpr int WAVE_SCRATCH = 16 * SYM_STRIDE + STAGE_PLANES * STAGE_STRIDE;   // phase 3, per wave: the transpose, then k / K of eight rows
static_assert(LIN_WAVES * WAVE_SCRATCH <= (LIN_COLS + NUM_SHARED_SCALARS) * LIN_TILE, "phase 3's scratch fits the region of the columns");
constexpr int ILQR_LDS_FLOATS = LIN_LDS_FLOATS + LIN_TILE * (PHI_STRIDE + PV_STRIDE);
static_assert(ILQR_LDS_FLOATS * sizeof(float) <= 160 * 1024, "fits a CU's LDS");
static_assert(D_T + 2 == 12 && NUM_LIN_DIRS + 2 == 16, "direction d <-> entry d + 2 of x: the states from 2, the controls from 12");
static_assert(LIN_TILE == 64 && LIN_WAVES == 8, "a wave owns eight rows of the tile");

typedef const IlqrArgs __attribute__((address_space(4))) *IlqrArgsC;

// d u'[k] / d clamp(a)[k]: control_lag's second term at action 1 (np_model_rollout_vjp.hip)
template <class A>
__device__ __forceinline__ float ilqr_lag_gain(const A &af, int k) {
    return k == 0 ? np_divc(((af.lag_new * 1.0f) * af.thrust_frac) * af.thrust_max, af.thrust_unit, af.r_thrust_unit) : (af.lag_new * 1.0f) * af.surf_max[k - 1];
}

// LDS traffic between the lanes of ONE wave: the DS instructions of a wave execute in order; this keeps the compiler from reordering them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// a caller's array as global memory (a generic pointer would be read with flat instructions), indexed in 64 bits
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T *glob(T *p) {
    return reinterpret_cast<__attribute__((address_space(1))) T *>(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ float lane_get(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ float pick4(int i, const float (&x)[4]) { return i == 0 ? x[0] : i == 1 ? x[1] : i == 2 ? x[2] : x[3]; }

// Qt = L diag(piv) L^T, unit lower L, row by row in this fixed order; x = -Qt^-1 b
struct Ldl4 {
    float l10, l20, l21, l30, l31, l32, piv[4];
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

// built for two waves per SIMD: one eight-wave workgroup per CU
__global__ __launch_bounds__(LIN_TILE * LIN_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_ilqr_backward_kernel(const IlqrArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[ILQR_LDS_FLOATS];
    float *blob = lds;
    const int t = (int)(threadIdx.x % LIN_TILE);
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LIN_TILE));
    float *col = lds + KBLOB_FLOATS + t;                   // this lane's columns, stride LIN_TILE
    float *shr = col + LIN_COLS * LIN_TILE;                // the tile's shared scalars, this lane's row
    float *phi = lds + LIN_LDS_FLOATS;                     // row r's Phi record at phi + r * PHI_STRIDE
    float *pv = phi + LIN_TILE * PHI_STRIDE;               // row r's vector state at pv + r * PV_STRIDE
    float *scr = lds + KBLOB_FLOATS + pw * WAVE_SCRATCH;   // phase 3: this wave's transpose area, then its staging area
    float *stage = scr + 16 * SYM_STRIDE;
    const int lg = t >> 4, lc = t & 15;                    // phase 3: the lane's place in the accumulator layout, rows 4 lg + r, column lc

    {  // the weight blob, once per workgroup: 16 bytes per thread and turn
        typedef const f32x4 __attribute__((address_space(1))) *gv4;
        const gv4 src = (gv4)(unsigned long long)a.kblob;
        f32x4 *dst = (f32x4 *)blob;
        for (int k = (int)threadIdx.x; k < KBLOB_FLOATS / 4; k += LIN_TILE * LIN_WAVES) dst[k] = src[k];
    }

    // this wave's directions, as in the linearisation: wave 0 the first, waves 1..6 two each, wave 7 the last (and the npos / epos columns)
    const int dir[2] = {pw == 0 ? 0 : 2 * pw - 1, (pw == 0 || pw == LIN_WAVES - 1) ? -1 : 2 * pw};
    const float qnan = __builtin_nanf("");
    const float r2d = (float)(180.0 / 3.141592653589793);
    IlqrArgsC ap = (IlqrArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    const long long tiles = (a.rows + LIN_TILE - 1) / LIN_TILE;
#pragma nounroll
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        NP_REREAD_ARGS(ap);
        const long long i = tile * LIN_TILE + t;
        const bool valid = i < ap->rows;
        const unsigned row = (unsigned)(valid ? i : ap->rows - 1);  // tail lanes shadow the last row; phase 3 skips their rows
        const unsigned own4 = row * 4u, src4 = (row / (unsigned)ap->fanout) * 4u;

        __syncthreads();  // the previous tile's last phase 3 has read its vectors
        if (pw == 0) {
            // ---- forward lag pre-pass: u_1..u_H of the tile into the workspace (np_model_rollout_vjp.hip) ----
            const unsigned act4 = row * (unsigned)ap->act_row_stride * 4u;
            float u[4];
#pragma unroll
            for (int k = 0; k < 4; k++) u[k] = at_off(ap->u0 + k * ap->ld0, src4);
#pragma nounroll
            for (int t0 = 0; t0 < ap->horizon; t0 += 4) {
                float act[4][4];
#pragma unroll
                for (int j = 0; j < 4; j++) {  // four steps' actions in flight together (past the end: the last step's again, unused)
                    const int tt = t0 + j < ap->horizon ? t0 + j : ap->horizon - 1;
                    const float *ab = ap->actions + (long long)tt * ap->act_step_stride;
#pragma unroll
                    for (int k = 0; k < 4; k++) act[j][k] = at_off(ab, act4 + 4u * k);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (t0 + j >= ap->horizon) break;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        float v = act[j][k];
                        v = v < -1.0f ? -1.0f : v;  // torch.clamp(action, -1, 1); NaN stays NaN
                        v = v > 1.0f ? 1.0f : v;
                        act[j][k] = v;
                    }
                    control_lag(ap->af, act[j], u);
                    if (valid) {
                        float *ub = ap->u_ws + (long long)(t0 + j) * 4 * ap->ld_traj;
#pragma unroll
                        for (int k = 0; k < 4; k++) at_off(ub + k * ap->ld_traj, own4) = u[k];
                    }
                }
            }
            // ---- the row's vector state at the end of the horizon: p = (0, g_u_end), dV = 0, running, not poisoned ----
            float *pr = pv + t * PV_STRIDE;
#pragma unroll
            for (int e = 0; e < PV_STRIDE; e++) pr[e] = 0.0f;
            if (ap->g_u_end) {
#pragma unroll
                for (int k = 0; k < 4; k++) pr[12 + k] = at_off(ap->g_u_end + k * ap->ld_traj, own4);
            }
            pr[PV_STOP] = __int_as_float(-1);
        }
        __threadfence_block();  // with the loop's first barrier: the workspace is visible to the tile's other waves

#pragma nounroll
        for (int step = ap->horizon - 1; step >= 0; step--) {
            bool ok;
            {
                __syncthreads();  // the blob, the workspace and the vectors are there; phase 3 of the previous step is through with its scratch

                NP_REREAD_ARGS(ap);
                // the linearisation point (s_step, u_{step+1}): the start or the recorded state, and the workspace
                const float *sb = step == 0 ? ap->s0 : ap->s_traj + (long long)(step - 1) * ap->traj_step_stride;
                const long long sld = step == 0 ? ap->ld0 : ap->ld_traj;
                const unsigned r4 = step == 0 ? src4 : own4;
                const float alpha = at_off(sb + 7 * sld, r4) * r2d, beta = at_off(sb + 8 * sld, r4) * r2d;
                const float el = at_off(ap->u_ws + ((long long)step * 4 + 1) * ap->ld_traj, own4);
                const float chk = ((alpha - alpha) + (beta - beta)) + (el - el);  // non-finite inputs poison the row (numerics spec)
                ok = (chk == chk);

                // ---- phase 1 ----
                float xn[NUM_NORM_GROUPS];
#pragma unroll
                for (int gi = 0; gi < NUM_NORM_GROUPS; gi++) {
                    const float v = (gi <= G_A_RUD) ? alpha : (gi <= G_B_O ? beta : el);
                    const float *h = blob + KBLOB_NORM_STRIDE * gi;  // (mean, sigma, RN(1 / sigma))
                    xn[gi] = np_divc(v - h[0], h[1], h[2]);
                }
                auto state = [&](int k) { return at_off(sb + k * sld, r4); };
                lin_phase1(pw, ap->af, blob, xn, col, shr, state);
            }

            __syncthreads();  // all 110 columns and the 12 shared scalars of the step are complete

            // ---- phase 2: this wave's columns of dt [A | B] into the rows' Phi records; p_s += g_s_traj[step] ----
            {
                NP_REREAD_ARGS(ap);
                const float *gs = ap->g_s_traj + (long long)step * ap->traj_step_stride;
                float gbar[2] = {0.0f, 0.0f}, gbar_ne[2] = {0.0f, 0.0f};
#pragma unroll
                for (int n = 0; n < 2; n++)
                    if (dir[n] >= 0 && dir[n] < D_T) gbar[n] = at_off(gs + (dir[n] + 2) * ap->ld_traj, own4);
                if (pw == LIN_WAVES - 1) {
                    gbar_ne[0] = at_off(gs, own4);
                    gbar_ne[1] = at_off(gs + ap->ld_traj, own4);
                }
                float s[12], u[4];
                {
                    const float *sb = step == 0 ? ap->s0 : ap->s_traj + (long long)(step - 1) * ap->traj_step_stride;
                    const long long sld = step == 0 ? ap->ld0 : ap->ld_traj;
                    const unsigned r4 = step == 0 ? src4 : own4;
#pragma unroll
                    for (int k = 0; k < 12; k++) s[k] = at_off(sb + k * sld, r4);
#pragma unroll
                    for (int k = 0; k < 4; k++) u[k] = at_off(ap->u_ws + ((long long)step * 4 + k) * ap->ld_traj, own4);
                }
                Jet<2> xd[12];
                nlplant_jets<2>(ap->af, s, u, shr, col, dir, ok, xd);
                const float dt = ap->dt;
                float *F = phi + t * PHI_STRIDE, *pr = pv + t * PV_STRIDE;
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    if (dir[n] < 0) continue;  // wave-uniform
                    const int e = dir[n] + 2;
#pragma unroll
                    for (int k = 0; k < 12; k++) F[k * 16 + e] = dt * ((ok || k < 6) ? xd[k].d[n] : qnan);  // a poisoned row: rows 6..11 are NaN
                    if (dir[n] < D_T) pr[e] = pr[e] + gbar[n];
                }
                if (pw == LIN_WAVES - 1) {  // nothing depends on npos and epos
#pragma unroll
                    for (int e = 0; e < 2; e++) {
#pragma unroll
                        for (int k = 0; k < 12; k++) F[k * 16 + e] = (ok || k < 6) ? 0.0f : qnan;
                        pr[e] = pr[e] + gbar_ne[e];
                    }
                }
                if (pw == 0 && !ok) pr[PV_POISON] = 1.0f;
            }

            __syncthreads();  // the Phi records and the vectors of the step are complete; the columns are dead

            // ---- phase 3: this wave's eight rows, one 16 x 16 matrix at a time ----
#if NPF16_ILQR_ONLY_PHASE != 12
            NP_REREAD_ARGS(ap);
#pragma nounroll
            for (int rr = 0; rr < 8; rr++) {
                const int rt = 8 * pw + rr;
                const long long grow = tile * LIN_TILE + rt;
                float k_own = 0.0f, K_own = 0.0f;  // what this lane stages: K entry 16 lg + lc, and k[lane] on lanes 0..3
                if (grow < ap->rows) {
                    const float *F = phi + rt * PHI_STRIDE;
                    float *pr = pv + rt * PV_STRIDE;
                    int stop = __builtin_amdgcn_readfirstlane(__float_as_int(pr[PV_STOP]));  // one address for the wave: uniform
                    bool poisoned = __builtin_amdgcn_readfirstlane(__float_as_int(pr[PV_POISON])) != 0;
                    float av[4], gin[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        av[k] = glob(ap->actions)[(long long)step * ap->act_step_stride + grow * ap->act_row_stride + k];
                        gin[k] = glob(ap->g_actions_in)[((long long)step * 4 + k) * ap->ld_traj + grow];
                    }
                    if (!poisoned && (av[0] != av[0] || av[1] != av[1] || av[2] != av[2] || av[3] != av[3])) {  // a NaN action gives a NaN row
                        poisoned = true;
                        if (t == 0) pr[PV_POISON] = 1.0f;
                    }
                    float Pn[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pn = 0.0f;
                    if (stop < 0 && !poisoned) {
                        // P in the accumulator layout (P = 0 at the end of the horizon), P_ss += diag(h_s[step])
                        float P[4], ph[4];
                        auto pw_row = glob(ap->p_ws) + grow * 256 + t;
                        const float hs = lc < 12 ? glob(ap->h_s)[step * 12 + lc] : 0.0f;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            P[r] = step == ap->horizon - 1 ? 0.0f : pw_row[r * 64];
                            const int ri = 4 * lg + r;
                            if (ri == lc) P[r] = P[r] + hs;
                            const float f = F[(ri < 12 ? ri : 11) * 16 + lc];
                            ph[r] = (ri < 12 ? f : 0.0f) + (ri == lc ? 1.0f : 0.0f);  // Phi[4 lg + r][lc]
                        }
                        // w = Phi^T p: w_c = p_c + sum_i dt [A | B][i][c] p_i, i ascending in one chain
                        float w = pr[lc];
#pragma unroll
                        for (int k = 0; k < 12; k++) w = fmaf(F[k * 16 + lc], pr[k], w);
                        f32x4 Y = {0.0f, 0.0f, 0.0f, 0.0f}, Wm = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int r = 0; r < 4; r++) Y = __builtin_amdgcn_mfma_f32_16x16x4f32(P[r], ph[r], Y, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; r++) Wm = __builtin_amdgcn_mfma_f32_16x16x4f32(ph[r], Y[r], Wm, 0, 0, 0);

                        const float kap = ap->af.lag_keep;
                        const float sc = lc < 12 ? 1.0f : kap, sr = lg == 3 ? kap : 1.0f;
                        float d[4], Wu[4], q[4][4], Qa[4], Qax[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            d[k] = (av[k] >= -1.0f && av[k] <= 1.0f) ? ilqr_lag_gain(ap->af, k) : 0.0f;
                            Wu[k] = __int_as_float(__builtin_amdgcn_ds_bpermute((48 + lc) * 4, __float_as_int(Wm[k])));  // W[12 + k][lc]
                        }
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            Qa[k] = d[k] * lane_get(w, 12 + k) + gin[k];
                            Qax[k] = d[k] * (sc * Wu[k]);
#pragma unroll
                            for (int j = 0; j <= k; j++) {  // the lower triangle of W_uu, mirrored
                                q[k][j] = (d[k] * d[j]) * lane_get(Wm[k], 60 + j) + (j == k ? ap->h_a[k] : 0.0f);
                                q[j][k] = q[k][j];
                            }
                        }
                        const float mu = ap->mu_rows ? glob(ap->mu_rows)[grow] : ap->mu;
                        Ldl4 f;
                        f.piv[0] = q[0][0] + mu;
                        f.l10 = q[1][0] / f.piv[0];
                        f.l20 = q[2][0] / f.piv[0];
                        f.l30 = q[3][0] / f.piv[0];
                        f.piv[1] = (q[1][1] + mu) - f.l10 * (f.l10 * f.piv[0]);
                        f.l21 = (q[2][1] - f.l20 * (f.l10 * f.piv[0])) / f.piv[1];
                        f.l31 = (q[3][1] - f.l30 * (f.l10 * f.piv[0])) / f.piv[1];
                        f.piv[2] = ((q[2][2] + mu) - f.l20 * (f.l20 * f.piv[0])) - f.l21 * (f.l21 * f.piv[1]);
                        f.l32 = ((q[3][2] - f.l30 * (f.l20 * f.piv[0])) - f.l31 * (f.l21 * f.piv[1])) / f.piv[2];
                        f.piv[3] = (((q[3][3] + mu) - f.l30 * (f.l30 * f.piv[0])) - f.l31 * (f.l31 * f.piv[1])) - f.l32 * (f.l32 * f.piv[2]);
                        const float inf = __builtin_inff();
                        bool bad = false;
#pragma unroll
                        for (int k = 0; k < 4; k++) bad = bad || !(f.piv[k] > 0.0f) || !(f.piv[k] < inf) || !(Qa[k] - Qa[k] == 0.0f);
                        if (bad) {  // the row stops here: zeros from this step down
                            stop = step;
                            if (t == 0) pr[PV_STOP] = __int_as_float(step);
                        } else {
                            float kv[4], Kc[4], G[4], v[4];
                            f.solve_neg(Qa, kv);
                            f.solve_neg(Qax, Kc);
                            float dv0 = 0.0f, dv1 = 0.0f, acc = sc * w;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const float qk = ((q[k][0] * kv[0] + q[k][1] * kv[1]) + q[k][2] * kv[2]) + q[k][3] * kv[3];
                                G[k] = (((q[k][0] * Kc[0] + q[k][1] * Kc[1]) + q[k][2] * Kc[2]) + q[k][3] * Kc[3]) + Qax[k];
                                v[k] = qk + Qa[k];
                                dv0 = dv0 + kv[k] * Qa[k];
                                dv1 = dv1 + kv[k] * qk;
                            }
#pragma unroll
                            for (int k = 0; k < 4; k++) acc = acc + Kc[k] * v[k];
#pragma unroll
                            for (int k = 0; k < 4; k++) acc = acc + Qax[k] * kv[k];
                            pn = acc;
                            f32x4 M;
#pragma unroll
                            for (int r = 0; r < 4; r++) M[r] = (sr * sc) * Wm[r];  // Q_xx = S W S
                            const float Kg = pick4(lg, Kc);
                            M = __builtin_amdgcn_mfma_f32_16x16x4f32(Kg, pick4(lg, G), M, 0, 0, 0);     // + K^T (Q_aa K + Q_ax)
                            M = __builtin_amdgcn_mfma_f32_16x16x4f32(pick4(lg, Qax), Kg, M, 0, 0, 0);   // + Q_ax^T K
                            wave_sync();
#pragma unroll
                            for (int r = 0; r < 4; r++) scr[(4 * lg + r) * SYM_STRIDE + lc] = M[r];
                            wave_sync();
#pragma unroll
                            for (int r = 0; r < 4; r++) Pn[r] = 0.5f * (M[r] + scr[lc * SYM_STRIDE + 4 * lg + r]);
                            K_own = Kg;
                            k_own = pick4(t & 3, kv);
                            wave_sync();
                            if (t == 0) {
                                pr[PV_DV] = pr[PV_DV] + dv0;
                                pr[PV_DV + 1] = pr[PV_DV + 1] + 0.5f * dv1;
                            }
                            if (lg == 0) pr[lc] = pn;
                            if (step > 0) {
#pragma unroll
                                for (int r = 0; r < 4; r++) pw_row[r * 64] = Pn[r];
                            }
                        }
                    }
                    const float fill = stop >= 0 ? 0.0f : qnan;  // a stopped row: zeros; a poisoned one: NaN
                    if (stop >= 0 || poisoned) k_own = K_own = fill;
                    if (step == 0) {  // the row's results at the start
                        const bool plain = stop < 0 && !poisoned;
                        auto o = glob(ap->dV) + grow;
                        if (t == 0) {
                            o[0] = plain ? pr[PV_DV] : fill;
                            o[ap->ld_out] = plain ? pr[PV_DV + 1] : fill;
                            glob(ap->status)[grow] = stop;
                        }
                        if (ap->p0) {
                            if (lg == 0) glob(ap->p0)[lc * ap->ld_out + grow] = plain ? pn : fill;
#pragma unroll
                            for (int r = 0; r < 4; r++) glob(ap->P0)[(long long)(64 * lg + 16 * r + lc) * ap->ld_out + grow] = plain ? Pn[r] : fill;
                        }
                    }
                }
                stage[t * STAGE_STRIDE + rr] = K_own;
                if (t < 4) stage[(64 + t) * STAGE_STRIDE + rr] = k_own;
            }
            // k and K of the wave's eight rows: 32-byte runs per plane
            wave_sync();
            {
                const int r8 = t & 7;
                const long long grow = tile * LIN_TILE + 8 * pw + r8;
#pragma unroll
                for (int it = 0; it < (STAGE_PLANES + 7) / 8; it++) {
                    const int plane = it * 8 + (t >> 3);
                    if (plane < STAGE_PLANES && grow < ap->rows) {
                        const float val = stage[plane * STAGE_STRIDE + r8];
                        if (plane < 64) glob(ap->K)[((long long)step * 64 + plane) * ap->ld_out + grow] = val;
                        else glob(ap->k)[((long long)step * 4 + (plane - 64)) * ap->ld_out + grow] = val;
                    }
                }
            }
#endif
        }
    }
}

hipError_t launch_model_ilqr_backward(int groups, const IlqrArgs &args, hipStream_t stream) {
    if (groups < 1 || args.rows < 1 || args.horizon < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_ilqr_backward_kernel, dim3((unsigned)groups), dim3(LIN_TILE * LIN_WAVES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
