// np_model_ekf.hip — a batched extended Kalman filter on the flight model: `horizon` predict + update steps of F16Model.update (reference
// envs/models/F16_model.py:51-67) per row and in ONE launch (np_f16_model_ekf).  With x = (s[12], u[0:4]) (np_model_ilqr.hip's coordinates),
// kappa and gain_k the control lag's factors, per step t from (s^, u^, P):
//     u' = kappa u^ + gain_k clamp(a_t, -1, 1);  xdot, A, B at (s^, u');  s- = s^ + dt xdot;  x- = (s-, u')          (update's own bits)
//     Phi = [[I + dt A, dt B], [0, I]];  S = diag(1 x 12, kappa x 4);  F = Phi S;  P- = sym(F P F^T) + diag(q)
//     n_i = 1 / r_i where bit i of `measure` is set and z_t[i] is finite, else 0;  nu_i = z_t[i] - x-_i there, else 0
//     W = I + P- N;  P+ = sym(W^-1 P-);  x+ = x- + P+ (N nu);  nis_t = sum_i n_i nu_i (z_t[i] - x+_i)
// (no n_i: P+ = P-, x+ = x- to the bit, no solve), in the equilibrated coordinates x = T x~ (T diagonal, powers of two from the host:
// P~ = T^-1 P T^-1, F~ = T^-1 F T, q~ = q / t^2, n~ = n t^2; every scaling is exact).  The mean stays in the caller's units, so that with
// no measurement it is the rollout's to the bit.  A row STOPS at step t (status[row] = t, its outputs the estimate entering step t) when a
// pivot of W is rejected or P+ is not finite; a row whose x- or P- is not finite (a non-finite alpha, beta or el, a NaN in P0, s0 or an
// action) is POISONED: NaN from that step on, status -1.  Neighbours are untouched either way.
//
// Schedule: the linearisation tile (64 rows, eight waves, the weight blob in LDS) persistent over a FORWARD loop whose linearisation
// point is the previous step's posterior.  A row's estimate x^ lives in LDS for the whole launch; nothing of it touches HBM between steps.
//   - phase 1 (a lane is a row): the lag on the row's action, then np_model_jets.h::lin_phase1 at (s^, u'): the 110 columns and the 12
//     shared scalars.  Wave 0 leaves u' in the row's x- record.
//   - phase 2 (a lane is a row): each wave pushes its two directions through nlplant_jets<2> and stores its two columns of dt [A | B] into
//     the row's Phi record in LDS (np_model_ilqr.hip's layout: 12 x 16 floats, stride 193); wave 0 adds the mean step s- = s^ + dt xdot to
//     the x- record; wave w brings planes 2 w and 2 w + 1 of z_t (coalesced; planes without a sensor are not read).
//   - phase 3: a WAVE IS A 16 x 16 COVARIANCE, in the accumulator layout of v_mfma_f32_16x16x4_f32 (np_model_mat16.h).  Wave w takes rows
//     8 w .. 8 w + 7 of the tile one at a time: P~ from the workspace (four coalesced 256-byte reads), F~^T from the Phi record (four LDS
//     reads per lane), P F^T and F (P F^T) as eight MFMAs, sym() through the wave's transpose area, W = I + P- N as one multiply per
//     register (a column scaling), the Gauss-Jordan solve on [W | P-] with the rows put back by one more product, sym() again; the
//     mat-vec P+ (N nu) as four butterflies over the 16 lanes of a group, nis as one more.  x+ goes back into the row's record, where the next
//     phase 1 linearises; P+ goes back to the workspace.  The per-step outputs of the wave's eight rows are staged in LDS and leave as
//     32-byte runs per plane.
//   - phase 3's LDS (transpose, staging) is the columns' region, dead between phase 2 and the next phase 1: three barriers per step, all in
//     workgroup-uniform control flow.  Stopped and poisoned rows are masked, never exited.
//   - after the last step the owning wave writes the row's final estimate: s, u from the record, P from the workspace (the same lanes that
//     wrote it), scaled back by T.
#include "np_model_ekf.h"

#include "np_model_jets.h"
#include "np_model_mat16.h"

namespace npf16 {

// Measurement builds only (tools/microbench/ekf_cost.py, the phase split): -DNPF16_EKF_ONLY_PHASE=12 leaves phase 3 out (the results are
// wrong).  0, the default, is the kernel.
#ifndef NPF16_EKF_ONLY_PHASE
#define NPF16_EKF_ONLY_PHASE 0
#endif

constexpr int EKF_PHI_STRIDE = 12 * 16 + 1;   // a row's Phi record: dt [A | B] as [12][16], padded to an odd stride
// a row's vector record: x^[16], x-[16], z_t[16], the stop step (int bits, -1 = running), the poison flag; an odd stride
constexpr int EKF_REC_STRIDE = 51, EKF_XM = 16, EKF_Z = 32, EKF_STOP = 48, EKF_POISON = 49;
constexpr int EKF_STAGE_PLANES = 16 + 16 + 1, EKF_STAGE_STRIDE = 9;   // x+, diag P+, nis of a wave's eight rows
constexpr int EKF_WAVE_SCRATCH = 16 * mat16::SYM_STRIDE + EKF_STAGE_PLANES * EKF_STAGE_STRIDE;
static_assert(LIN_WAVES * EKF_WAVE_SCRATCH <= (LIN_COLS + NUM_SHARED_SCALARS) * LIN_TILE, "phase 3's scratch fits the region of the columns");
constexpr int EKF_LDS_FLOATS = LIN_LDS_FLOATS + LIN_TILE * (EKF_PHI_STRIDE + EKF_REC_STRIDE);
static_assert(EKF_LDS_FLOATS * sizeof(float) <= 160 * 1024, "fits a CU's LDS");
static_assert(D_T + 2 == 12 && NUM_LIN_DIRS + 2 == 16, "direction d <-> entry d + 2 of x: the states from 2, the controls from 12");
static_assert(LIN_TILE == 64 && LIN_WAVES == 8, "a wave owns eight rows of the tile");

typedef const EkfArgs __attribute__((address_space(4))) *EkfArgsC;

namespace ekf {

using namespace mat16;

// the sum over the 16 lanes of a group (the columns of a row): the same bits in every lane
__device__ __forceinline__ float group_sum(float v, int lane) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v = v + from_lane(v, lane ^ m);
    return v;
}

// One step of one row on one wave.  R: the row's vector record, F: its Phi record, pw_row: its place in the workspace (this lane's first
// entry), scr: the wave's transpose area.  Returns what the lane stages: x+_c, (P+)_cc and nis, NaN for a row that does not run.
__device__ __forceinline__ void row_step(float *R, const float *F, __attribute__((address_space(1))) float *pw_row, float *scr, EkfArgsC ap,
                                         long long grow, int step, int lane, float &x_own, float &pd_own, float &nis_own) {
    const int g = lane >> 4, c = lane & 15;
    const float qnan = __builtin_nanf("");
    x_own = pd_own = nis_own = qnan;
    const int stop = __builtin_amdgcn_readfirstlane(__float_as_int(R[EKF_STOP]));   // one address for the wave: uniform
    const bool poisoned = __builtin_amdgcn_readfirstlane(__float_as_int(R[EKF_POISON])) != 0;
    if (stop >= 0 || poisoned) return;

    const float tc = ap->t[c], tic = ap->tinv[c];
    f32x4 P, Ft;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int j = 4 * g + r;
        P[r] = step == 0 ? (glob(ap->P0)[(long long)(16 * j + c) * ap->ld + grow] * ap->tinv[j]) * tic : pw_row[r * 64];
        const float f = F[(c < 12 ? c : 11) * 16 + j];
        const float phi = (c < 12 ? f : 0.0f) + (c == j ? 1.0f : 0.0f);   // Phi[c][4 g + r]
        Ft[r] = ((phi * (j < 12 ? 1.0f : ap->kappa)) * ap->t[j]) * tic;   // F~^T[4 g + r][c] = (T^-1 Phi S T)[c][4 g + r]
    }
    // P- = sym(F P F^T) + diag(q): P symmetric, so mm(P, Ft) = P F^T, and mm(Ft, .) multiplies by F from the left
    f32x4 Pm = sym_half(mm(Ft, mm(P, Ft)), scr, g, c);
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (4 * g + r == c) Pm[r] = Pm[r] + ap->q[c];
    const float xm = R[EKF_XM + c];
    if (wave_any(!finite4(Pm) || !(xm - xm == 0.0f))) {   // nothing to filter: NaN from here on
        if (lane == 0) R[EKF_POISON] = 1.0f;
        return;
    }
    const float zc = R[EKF_Z + c];
    const bool measured = ((ap->measure >> c) & 1) != 0 && zc - zc == 0.0f;
    const float nt = measured ? ap->nt[c] : 0.0f, rinv = measured ? ap->rinv[c] : 0.0f, nu = measured ? zc - xm : 0.0f;
    f32x4 Pp = Pm;
    float xp = xm, nis = 0.0f;
    if (wave_any(measured)) {
        f32x4 W, X = Pm, PT;
#pragma unroll
        for (int r = 0; r < 4; r++) W[r] = (4 * g + r == c ? 1.0f : 0.0f) + Pm[r] * nt;
        bool bad = solve(W, X, PT, g, c) != 0;
        if (!bad) {
            Pp = sym_half(mm(PT, X), scr, g, c);   // the rows back in order, then sym()
            bad = wave_any(!finite4(Pp));
        }
        if (bad) {   // the row stops here with the estimate it came in with
            if (lane == 0) R[EKF_STOP] = __int_as_float(step);
            if (step == 0) {
#pragma unroll
                for (int r = 0; r < 4; r++) pw_row[r * 64] = P[r];
            }
            return;
        }
        // x+ = x- + T (P~+ (n~ nu~)): the lanes of group g reduce rows 4 g .. 4 g + 3
        const float wv = nt * (nu * tic);
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; r++) y[r] = group_sum(Pp[r] * wv, lane);
        wave_sync();
        if (c == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++) R[4 * g + r] = R[EKF_XM + 4 * g + r] + ap->t[4 * g + r] * y[r];
        }
        wave_sync();
        xp = R[c];
        nis = group_sum(measured ? (rinv * nu) * (zc - xp) : 0.0f, lane);
    } else {
        wave_sync();
        if (g == 0) R[c] = xm;
        wave_sync();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) pw_row[r * 64] = Pp[r];
    x_own = xp;
    pd_own = (from_lane(pick4(c & 3, Pp), 16 * (c >> 2) + c) * tc) * tc;
    nis_own = nis;
}

}  // namespace ekf

// built for two waves per SIMD: one eight-wave workgroup per CU
__global__ __launch_bounds__(LIN_TILE * LIN_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_ekf_kernel(const EkfArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[EKF_LDS_FLOATS];
    float *blob = lds;
    const int t = (int)(threadIdx.x % LIN_TILE);
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LIN_TILE));
    float *phi = lds + LIN_LDS_FLOATS;                         // row r's Phi record at phi + r * EKF_PHI_STRIDE
    float *rec = phi + LIN_TILE * EKF_PHI_STRIDE;              // row r's vector record at rec + r * EKF_REC_STRIDE
    float *scr = lds + KBLOB_FLOATS + pw * EKF_WAVE_SCRATCH;   // phase 3: this wave's transpose area, then its staging area
    float *stage = scr + 16 * mat16::SYM_STRIDE;

    {  // the weight blob, once per workgroup: 16 bytes per thread and turn
        typedef const f32x4 __attribute__((address_space(1))) *gv4;
        const gv4 src = (gv4)(unsigned long long)a.kblob;
        f32x4 *dst = (f32x4 *)blob;
        for (int k = (int)threadIdx.x; k < KBLOB_FLOATS / 4; k += LIN_TILE * LIN_WAVES) dst[k] = src[k];
    }

    // What a phase derives from the lane or the wave index — its places in LDS, the 0 / 1 seeds of the directions, the masks of the
    // accumulator layout — is made again per phase behind an opaque statement: left loop-invariant it is all hoisted out of the step loop
    // and lives in VGPRs across the nets (np_model_trim.hip).
#define EKF_LANE(tp)       \
    int tp = t;            \
    asm volatile("" : "+v"(tp)); \
    float *my = rec + tp * EKF_REC_STRIDE;        /* this lane's row: its vector record */ \
    float *col = lds + KBLOB_FLOATS + tp;         /* its columns, stride LIN_TILE */ \
    float *shr = col + LIN_COLS * LIN_TILE        /* the tile's shared scalars, its row */
    const float qnan = __builtin_nanf("");
    const float r2d = (float)(180.0 / 3.141592653589793);
    EkfArgsC ap = (EkfArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    const long long tiles = (a.rows + LIN_TILE - 1) / LIN_TILE;
#pragma nounroll
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        NP_REREAD_ARGS(ap);
        const long long i = tile * LIN_TILE + t;
        const unsigned row = (unsigned)(i < ap->rows ? i : ap->rows - 1);  // tail lanes shadow the last row; phase 3 skips their rows
        const unsigned own4 = row * 4u;

        __syncthreads();  // every wave is done with the previous tile's records
        {
            EKF_LANE(tp);
            (void)shr;
#pragma unroll
        for (int n = 0; n < 2; n++) {  // the start: wave w brings entries 2 w and 2 w + 1 of x^
            const int e = 2 * pw + n;
            my[e] = e < 12 ? at_off(ap->s0 + e * ap->ld0, own4) : at_off(ap->u0 + (e - 12) * ap->ld0, own4);
        }
            if (pw == 0) {
                my[EKF_STOP] = __int_as_float(-1);
                my[EKF_POISON] = 0.0f;
            }
        }

#pragma nounroll
        for (int step = 0; step < ap->horizon; step++) {
            __syncthreads();  // the blob and the estimates are there; phase 3 of the previous step is through with its scratch
            {
                NP_REREAD_ARGS(ap);
                EKF_LANE(tp);
                // ---- the lag on the row's action, then phase 1 at (s^, u') ----
                const unsigned act4 = row * (unsigned)ap->act_row_stride * 4u;
                const float *ab = ap->actions + (long long)step * ap->act_step_stride;
                float act[4], u[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float v = at_off(ab, act4 + 4u * k);
                    v = v < -1.0f ? -1.0f : v;  // torch.clamp(action, -1, 1); NaN stays NaN
                    v = v > 1.0f ? 1.0f : v;
                    act[k] = v;
                    u[k] = my[12 + k];
                }
                control_lag(ap->af, act, u);
                if (pw == 0) {
#pragma unroll
                    for (int k = 0; k < 4; k++) my[EKF_XM + 12 + k] = u[k];
                }
                const float alpha = my[7] * r2d, beta = my[8] * r2d, el = u[1];
                float xn[NUM_NORM_GROUPS];
#pragma unroll
                for (int gi = 0; gi < NUM_NORM_GROUPS; gi++) {
                    const float v = (gi <= G_A_RUD) ? alpha : (gi <= G_B_O ? beta : el);
                    const float *h = blob + KBLOB_NORM_STRIDE * gi;  // (mean, sigma, RN(1 / sigma))
                    xn[gi] = np_divc(v - h[0], h[1], h[2]);
                }
                auto state = [&](int k) { return my[k]; };
                lin_phase1(pw, ap->af, blob, xn, col, shr, state);
            }

            __syncthreads();  // all 110 columns, the 12 shared scalars and u' of the step are complete

            // ---- phase 2: this wave's columns of dt [A | B] into the rows' Phi records; the mean step; this wave's planes of z ----
            {
                NP_REREAD_ARGS(ap);
                EKF_LANE(tp);
                // this wave's directions, as in the linearisation: wave 0 the first (and xdot), waves 1..6 two each, wave 7 the last
                int w_ = pw;
                asm volatile("" : "+s"(w_));
                const int dir[2] = {w_ == 0 ? 0 : 2 * w_ - 1, (w_ == 0 || w_ == LIN_WAVES - 1) ? -1 : 2 * w_};
                float zin[2];
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    const int e = 2 * pw + n;
                    zin[n] = ((ap->measure >> e) & 1) ? at_off(ap->z + ((long long)step * 16 + e) * ap->ld, own4) : qnan;  // wave-uniform
                }
                float s[12], u[4];
#pragma unroll
                for (int k = 0; k < 12; k++) s[k] = my[k];
#pragma unroll
                for (int k = 0; k < 4; k++) u[k] = my[EKF_XM + 12 + k];
                const float alpha = s[7] * r2d, beta = s[8] * r2d;
                const float chk = ((alpha - alpha) + (beta - beta)) + (u[1] - u[1]);  // non-finite inputs poison the row (numerics spec)
                const bool ok = (chk == chk);
                Jet<2> xd[12];
                nlplant_jets<2>(ap->af, s, u, shr, col, dir, ok, xd);
                const float dt = ap->dt;
                float *F = phi + tp * EKF_PHI_STRIDE;
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    my[EKF_Z + 2 * pw + n] = zin[n];
                    if (dir[n] < 0) continue;  // wave-uniform
                    const int e = dir[n] + 2;
#pragma unroll
                    for (int k = 0; k < 12; k++) F[k * 16 + e] = dt * ((ok || k < 6) ? xd[k].d[n] : qnan);  // a poisoned row: rows 6..11 are NaN
                }
                if (pw == LIN_WAVES - 1) {  // nothing depends on npos and epos
#pragma unroll
                    for (int e = 0; e < 2; e++) {
#pragma unroll
                        for (int k = 0; k < 12; k++) F[k * 16 + e] = (ok || k < 6) ? 0.0f : qnan;
                    }
                }
                if (pw == 0) {  // update's Euler step on the tile's xdot: the rollout's own expression
#pragma unroll
                    for (int k = 0; k < 12; k++) my[EKF_XM + k] = s[k] + dt * xd[k].v;
                }
            }

            __syncthreads();  // the Phi records, x- and z of the step are complete; the columns are dead

            // ---- phase 3: this wave's eight rows, one 16 x 16 covariance at a time ----
#if NPF16_EKF_ONLY_PHASE != 12
            NP_REREAD_ARGS(ap);
            int tl = t;
            asm volatile("" : "+v"(tl));
#pragma nounroll
            for (int rr = 0; rr < 8; rr++) {
                const int rt = 8 * pw + rr;
                const long long grow = tile * LIN_TILE + rt;
                float x_own = qnan, pd_own = qnan, nis_own = qnan;
                if (grow < ap->rows)
                    ekf::row_step(rec + rt * EKF_REC_STRIDE, phi + rt * EKF_PHI_STRIDE, mat16::glob(ap->p_ws) + grow * 256 + tl, scr, ap, grow, step, tl,
                                  x_own, pd_own, nis_own);
                if (tl < 16) stage[tl * EKF_STAGE_STRIDE + rr] = x_own;
                else if (tl < 32) stage[tl * EKF_STAGE_STRIDE + rr] = pd_own;
                else if (tl == 32) stage[32 * EKF_STAGE_STRIDE + rr] = nis_own;
            }
            // the per-step outputs of the wave's eight rows: 32-byte runs per plane
            mat16::wave_sync();
            {
                const int r8 = tl & 7;
                const long long grow = tile * LIN_TILE + 8 * pw + r8;
#pragma unroll
                for (int it = 0; it < (EKF_STAGE_PLANES + 7) / 8; it++) {
                    const int plane = it * 8 + (tl >> 3);
                    if (plane < EKF_STAGE_PLANES && grow < ap->rows) {
                        const float val = stage[plane * EKF_STAGE_STRIDE + r8];
                        if (plane < 16) {
                            if (ap->x_traj) mat16::glob(ap->x_traj)[((long long)step * 16 + plane) * ap->ld_out + grow] = val;
                        } else if (plane < 32) {
                            if (ap->pdiag_traj) mat16::glob(ap->pdiag_traj)[((long long)step * 16 + (plane - 16)) * ap->ld_out + grow] = val;
                        } else if (ap->nis) {
                            mat16::glob(ap->nis)[(long long)step * ap->ld_out + grow] = val;
                        }
                    }
                }
            }
#endif
        }

        // ---- the final estimate of the wave's eight rows: the record, and the workspace scaled back by T ----
#if NPF16_EKF_ONLY_PHASE != 12
        NP_REREAD_ARGS(ap);
        int tf = t;
        asm volatile("" : "+v"(tf));
        const int lg = tf >> 4, lc = tf & 15;
#pragma nounroll
        for (int rr = 0; rr < 8; rr++) {
            const int rt = 8 * pw + rr;
            const long long grow = tile * LIN_TILE + rt;
            if (grow >= ap->rows) continue;  // wave-uniform
            const float *R = rec + rt * EKF_REC_STRIDE;
            const int stop = __builtin_amdgcn_readfirstlane(__float_as_int(R[EKF_STOP]));
            const bool poisoned = __builtin_amdgcn_readfirstlane(__float_as_int(R[EKF_POISON])) != 0;
            const float x = poisoned ? qnan : R[lc];
            if (tf < 12) mat16::glob(ap->s_out)[(long long)tf * ap->ld_out + grow] = x;
            else if (tf < 16) mat16::glob(ap->u_out)[(long long)(tf - 12) * ap->ld_out + grow] = x;
            else if (tf == 16) mat16::glob(ap->u_out)[4 * ap->ld_out + grow] = mat16::glob(ap->u0)[4 * ap->ld0 + grow];  // lef is handed through
            else if (tf == 17) mat16::glob(ap->status)[grow] = poisoned ? -1 : stop;
            auto pw_row = mat16::glob(ap->p_ws) + grow * 256 + tf;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = 4 * lg + r;
                const float p = poisoned ? qnan : (pw_row[r * 64] * ap->t[j]) * ap->t[lc];
                mat16::glob(ap->P_out)[(long long)(16 * j + lc) * ap->ld_out + grow] = p;
            }
        }
#endif
    }
}

hipError_t launch_model_ekf(int groups, const EkfArgs &args, hipStream_t stream) {
    if (groups < 1 || args.rows < 1 || args.horizon < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_ekf_kernel, dim3((unsigned)groups), dim3(LIN_TILE * LIN_WAVES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
