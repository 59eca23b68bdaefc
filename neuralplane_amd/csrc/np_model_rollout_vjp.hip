// np_model_rollout_vjp.hip — the open-loop rollout differentiated: the vector-Jacobian product of H Euler applications of F16Model.update
// (reference envs/models/F16_model.py:51-67) with respect to the action sequence and the start, per row and in ONE launch
// (np_f16_model_rollout_vjp).  One model step is
//     u_{t+1} = lag_keep u_t + gain_k clamp(a_t, -1, 1)          (np_f16_device.h::control_lag)
//     s_{t+1} = s_t + dt f(s_t, u_{t+1})                         (nlplant)
// and with cotangents gbar_t on the recorded states s_1..s_H and gbar_u on u_H the sweep runs t = H-1 .. 0:
//     ls = cotangent of s_{t+1} (gbar_{t+1} + what step t + 1 handed back)
//     mu = lu + dt B(s_t, u_{t+1})^T ls        g_a[t] = 1[-1 <= a_t <= 1] gain mu        lu <- lag_keep mu
//     ls <- gbar_t + (ls + dt A(s_t, u_{t+1})^T ls)
// ending in g_s0 = ls, g_u0[0:4] = lu, g_u0[4] = gbar_u[4] (lef is handed through).  The linearisation points are the states the rollout
// recorded (fp32): nothing is integrated again.  A pure function: nothing of the context is written.
//
// Schedule: the linearisation kernel's tile (np_model_linearize.hip) made persistent over the reverse loop.  Eight waves share a 64-row
// tile, the single-set weight blob sits in LDS once per workgroup, a workgroup walks the tiles blockIdx.x, + gridDim.x, ...  Per tile:
//   - forward lag pre-pass (wave 0): the lag is linear and cheap, so u_1..u_H are computed forward with control_lag itself on the clamped
//     actions — the rollout's bits — and written to the caller's workspace u_ws [H][4][ld]: 16 B read and 16 B written per row and step,
//     four steps' actions in flight at a time.  (Recomputing the prefix per step would be O(H^2); inverting the lag is not bit-exact.)  A
//     block-scope fence and the first barrier of the loop make it visible to the other waves.
//   - per reverse step, phase 1: the 110 columns (42 net values + 68 input derivatives) by PLAN8_LIN and the 12 shared scalars, to LDS,
//     exactly as the linearisation does it (np_model_jets.h::lin_phase1).
//   - one barrier.
//   - phase 2: each wave pushes its two directions through nlplant_jets<2> and contracts on the spot, c_j = sum_k ls[k] xd[k].d[j], k
//     ascending in ONE FMA chain: no wave stores 12 numbers per column.
//   - the adjoint (ls[12], lu[4]) lives in LDS as per-lane columns, 16 x 64 floats, DOUBLE-BUFFERED: the kernel the tile comes from sits at
//     220 VGPRs at two waves per SIMD, and sixteen more values live across both phases would go to scratch.  In step t every wave reads the
//     old buffer and writes only its own directions' entries of the other: ls_new[j] for a state direction (plus the recorded state's
//     cotangent gbar_t[j], one coalesced load per direction issued at the head of phase 2 ahead of the state's own loads: its latency
//     hides behind the equations of motion and it is not live across the nets), lu_new[k] and the global store of g_a[t][k] for a control
//     direction.  Wave 7 carries the two components of the structurally zero npos / epos columns.  The last step (t = 0) stores g_s0 and
//     g_u0 instead.  Two barriers per step, the two the linearisation loop has; there is no third phase.
//   - a held action (act_step_stride = 0): the owning waves accumulate g_a over the steps, t descending, and store once.
//   - a non-finite alpha, beta or el at some step poisons that row as poison_jet does in the linearisation (rows 6..11 of every column
//     of [A | B] are NaN): the row's adjoint, and with it its outputs, become NaN; its neighbours are untouched.
// Matrix instructions are not used, for the reasons at the head of np_model_linearize.hip: layers 20 / 10 / 5 wide with per-row ReLU masks
// pad badly into 16 x 16 or 32 x 32 tiles, and the value chains must keep the spec's order so that the ReLU decisions are the forward pass's.
#include "np_model_rollout_vjp.h"

#include "np_model_jets.h"

namespace npf16 {

// Measurement builds only (tools/microbench/rollout_vjp_cost.py, the phase split): -DNPF16_VJP_ONLY_PHASE=1 / 2 leaves the OTHER phase's
// arithmetic out — the loop, its barriers and its loads stay, the results are wrong.  0, the default, is the kernel.
#ifndef NPF16_VJP_ONLY_PHASE
#define NPF16_VJP_ONLY_PHASE 0
#endif

constexpr int VJP_ADJ = 16;                                               // ls[12] then lu[4]: entry of direction d is d + 2
constexpr int VJP_LDS_FLOATS = LIN_LDS_FLOATS + 2 * VJP_ADJ * LIN_TILE;   // blob + columns + shared scalars (88 KB) + two adjoint buffers (8 KB)
static_assert(VJP_LDS_FLOATS * sizeof(float) <= 160 * 1024, "fits a CU's LDS");
static_assert(D_T + 2 == 12 && NUM_LIN_DIRS + 2 == VJP_ADJ, "direction d <-> adjoint entry d + 2: the states from 2, the controls from 12");

typedef const RolloutVjpArgs __attribute__((address_space(4))) *VjpArgsC;

// d u_{t+1}[k] / d clamp(a_t)[k]: control_lag's second term, which is linear in the action, at action 1 (the same operations)
template <class A>
__device__ __forceinline__ float lag_gain(const A &af, int k) {
    return k == 0 ? np_divc(((af.lag_new * 1.0f) * af.thrust_frac) * af.thrust_max, af.thrust_unit, af.r_thrust_unit) : (af.lag_new * 1.0f) * af.surf_max[k - 1];
}

// built for two waves per SIMD: one eight-wave workgroup per CU (96 KB of its LDS)
__global__ __launch_bounds__(LIN_TILE * LIN_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_rollout_vjp_kernel(const RolloutVjpArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[VJP_LDS_FLOATS];
    float *blob = lds;
    const int t = (int)(threadIdx.x % LIN_TILE);
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LIN_TILE));
    float *col = lds + KBLOB_FLOATS + t;                   // this lane's columns, stride LIN_TILE
    float *shr = col + LIN_COLS * LIN_TILE;                // the tile's shared scalars, this lane's row
    float *adj = shr + NUM_SHARED_SCALARS * LIN_TILE;      // this lane's adjoint: entry e of buffer b at adj[(b * VJP_ADJ + e) * LIN_TILE]

    {  // the weight blob, once per workgroup: 16 bytes per thread and turn
        typedef const f32x4 __attribute__((address_space(1))) *gv4;
        const gv4 src = (gv4)(unsigned long long)a.kblob;
        f32x4 *dst = (f32x4 *)blob;
        for (int k = (int)threadIdx.x; k < KBLOB_FLOATS / 4; k += LIN_TILE * LIN_WAVES) dst[k] = src[k];
    }

    // this wave's directions, as in the linearisation: wave 0 the first, waves 1..6 two each, wave 7 the last (and the npos / epos entries)
    const int dir[2] = {pw == 0 ? 0 : 2 * pw - 1, (pw == 0 || pw == LIN_WAVES - 1) ? -1 : 2 * pw};
    const float qnan = __builtin_nanf("");
    const float r2d = (float)(180.0 / 3.141592653589793);
    // the launch's arguments are read through the kernel-argument segment behind an opaque statement per phase (np_model_linearize.hip)
    VjpArgsC ap = (VjpArgsC)__builtin_amdgcn_kernarg_segment_ptr();
    int wr = 0;  // the adjoint buffer the next write goes to; the one nobody reads in the step at hand (it runs on from tile to tile)

    const long long tiles = (a.rows + LIN_TILE - 1) / LIN_TILE;
#pragma nounroll
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        NP_REREAD_ARGS(ap);
        const long long i = tile * LIN_TILE + t;
        const bool valid = i < ap->rows;
        const unsigned row = (unsigned)(valid ? i : ap->rows - 1);  // tail lanes shadow the last row; their stores are masked
        const unsigned own4 = row * 4u, src4 = (row / (unsigned)ap->fanout) * 4u;
        const bool held = ap->act_step_stride == 0;

        // ---- forward lag pre-pass: u_1..u_H of the tile into the workspace ----
        if (pw == 0) {
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
        }
        __threadfence_block();  // with the loop's first barrier: the workspace is visible to the tile's other waves

        // ---- the adjoint at the end of the horizon: each wave its own entries, gbar_H and gbar_u ----
        {
            float *w = adj + wr * VJP_ADJ * LIN_TILE;
            const float *gs = ap->g_s_traj + (long long)(ap->horizon - 1) * ap->traj_step_stride;
#pragma unroll
            for (int n = 0; n < 2; n++) {
                if (dir[n] < 0) continue;  // wave-uniform
                const int e = dir[n] + 2;
                w[e * LIN_TILE] = dir[n] < D_T ? at_off(gs + e * ap->ld_traj, own4) : ap->g_u_end ? at_off(ap->g_u_end + (dir[n] - D_T) * ap->ld_traj, own4) : 0.0f;
            }
            if (pw == LIN_WAVES - 1) {
                w[0] = at_off(gs, own4);
                w[LIN_TILE] = at_off(gs + ap->ld_traj, own4);
            }
        }
        float acc[2] = {0.0f, 0.0f};  // a held action's gradient, summed over the steps (control directions only)

#pragma nounroll
        for (int step = ap->horizon - 1; step >= 0; step--) {
            const int rd = wr;
            wr ^= 1;
            bool ok;
            {
                __syncthreads();  // the blob and the workspace are there (first step of a tile); every wave has read the previous step's columns

                NP_REREAD_ARGS(ap);
                // the linearisation point (s_step, u_{step+1}): the start or the recorded state, and the workspace
                const float *sb = step == 0 ? ap->s0 : ap->s_traj + (long long)(step - 1) * ap->traj_step_stride;
                const long long sld = step == 0 ? ap->ld0 : ap->ld_traj;
                const unsigned r4 = step == 0 ? src4 : own4;
                const float alpha = at_off(sb + 7 * sld, r4) * r2d, beta = at_off(sb + 8 * sld, r4) * r2d;
                const float el = at_off(ap->u_ws + ((long long)step * 4 + 1) * ap->ld_traj, own4);
                const float chk = ((alpha - alpha) + (beta - beta)) + (el - el);  // non-finite inputs poison every coefficient (numerics spec)
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
#if NPF16_VJP_ONLY_PHASE != 2
                lin_phase1(pw, ap->af, blob, xn, col, shr, state);
#else
                if (xn[0] == 12345.0f) col[0] = state(4);  // keeps the loads and the normalisation alive
#endif
            }

            __syncthreads();  // all 110 columns and the 12 shared scalars of the step are complete; so is the adjoint the last step wrote

            // ---- phase 2 ----
            NP_REREAD_ARGS(ap);
            const float *lam = adj + rd * VJP_ADJ * LIN_TILE;
            float *nxt = adj + wr * VJP_ADJ * LIN_TILE;
            // the cotangent of the recorded state s_step, this wave's entries (s_0 is not recorded: none)
            float gbar[2] = {0.0f, 0.0f}, gbar_ne[2] = {0.0f, 0.0f};
            if (step > 0) {
                const float *gs = ap->g_s_traj + (long long)(step - 1) * ap->traj_step_stride;
#pragma unroll
                for (int n = 0; n < 2; n++)
                    if (dir[n] >= 0 && dir[n] < D_T) gbar[n] = at_off(gs + (dir[n] + 2) * ap->ld_traj, own4);
                if (pw == LIN_WAVES - 1) {
                    gbar_ne[0] = at_off(gs, own4);
                    gbar_ne[1] = at_off(gs + ap->ld_traj, own4);
                }
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
#if NPF16_VJP_ONLY_PHASE != 1
            nlplant_jets<2>(ap->af, s, u, shr, col, dir, ok, xd);
#else
#pragma unroll
            for (int k = 0; k < 12; k++) xd[k].d[0] = xd[k].d[1] = s[k] + u[k & 3];  // the loads stay; the equations of motion do not
#endif
            const float dt = ap->dt;
#pragma unroll
            for (int n = 0; n < 2; n++) {
                if (dir[n] < 0) continue;  // wave-uniform
                // c = column dir[n] of [A | B] against ls: k ascending, one chain.  A non-finite alpha, beta or el: rows 6..11 are NaN, as the linearisation stores them
                float c = lam[0] * xd[0].d[n];
#pragma unroll
                for (int k = 1; k < 12; k++) c = fmaf(lam[k * LIN_TILE], (ok || k < 6) ? xd[k].d[n] : qnan, c);
                const int e = dir[n] + 2;
                const float into = lam[e * LIN_TILE] + dt * c;
                if (dir[n] < D_T) {  // a state direction: ls_new[j]
                    const float v = into + gbar[n];
                    if (step > 0) nxt[e * LIN_TILE] = v;
                    else if (valid) at_off(ap->g_s0 + e * ap->ld_out, own4) = v;
                } else {             // a control direction: mu -> g_a[step][k] and lu_new[k]
                    const int k = dir[n] - D_T;
                    const unsigned act4 = row * (unsigned)ap->act_row_stride * 4u + 4u * k;
                    const float av = at_off(ap->actions + (long long)step * ap->act_step_stride, act4);
                    // torch.clamp's backward: the gradient passes on [-1, 1], ends included; a NaN action gives NaN
                    const float ga = (av >= -1.0f && av <= 1.0f) ? lag_gain(ap->af, k) * into : (av != av ? qnan : 0.0f);
                    if (held) acc[n] = acc[n] + ga;
                    else if (valid) at_off(ap->g_actions + (long long)step * ap->act_step_stride, act4) = ga;
                    const float lu = ap->af.lag_keep * into;
                    if (step > 0) nxt[e * LIN_TILE] = lu;
                    else if (valid) at_off(ap->g_u0 + k * ap->ld_out, own4) = lu;
                }
            }
            if (pw == LIN_WAVES - 1) {  // nothing depends on npos and epos: their columns are zero (NaN in rows 6..11 of a poisoned row)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const float v = (ok ? lam[e * LIN_TILE] : qnan) + gbar_ne[e];
                    if (step > 0) nxt[e * LIN_TILE] = v;
                    else if (valid) at_off(ap->g_s0 + e * ap->ld_out, own4) = v;
                }
            }
        }

        NP_REREAD_ARGS(ap);
        if (valid) {
            if (held) {
#pragma unroll
                for (int n = 0; n < 2; n++)
                    if (dir[n] >= D_T) at_off(ap->g_actions, row * (unsigned)ap->act_row_stride * 4u + 4u * (dir[n] - D_T)) = acc[n];
            }
            if (pw == LIN_WAVES - 1)  // lef is not F16Model.update's business: handed through
                at_off(ap->g_u0 + 4 * ap->ld_out, own4) = ap->g_u_end ? at_off(ap->g_u_end + 4 * ap->ld_traj, own4) : 0.0f;
        }
    }
}

hipError_t launch_model_rollout_vjp(int groups, const RolloutVjpArgs &args, hipStream_t stream) {
    if (groups < 1 || args.rows < 1 || args.horizon < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_rollout_vjp_kernel, dim3((unsigned)groups), dim3(LIN_TILE * LIN_WAVES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
