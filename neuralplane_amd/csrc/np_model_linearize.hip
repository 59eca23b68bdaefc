// np_model_linearize.hip — the flight model's linearisation about a flight condition, per row and in ONE launch (np_f16_model_linearize):
//     xdot = f(s, u),   A = df/ds [12][12],   B = df/du [12][4]
// of F16Dynamics.nlplant (reference envs/models/F16/F16_dynamics.py:37-228), s the 12 states and u the four lagged controls nlplant reads.
// A pure function of (s, u): nothing of the context is written.  xdot is the spec's operations in the spec's order (np_f16_device.h::nlplant,
// restated here on value + tangent pairs whose value halves are those very operations): bit-identical to the oracle and to the step kernels.
//
// Why analytic: each of the 42 live nets has 1-3 inputs (alpha, beta, el), so ONE pass over a net's weights gives its value and its 1-3 input
// derivatives (forward mode: a tangent chain beside the value chain, 68 tangent outputs in all); the rest is the chain rule through closed-form
// code.  Finite differences need ~28 model evaluations per row and break wherever a step straddles one of the nets' 1 405 ReLU kinks.
//
// Schedule.  One lane = one row of a 64-row tile; eight waves share the tile; a workgroup walks the tiles blockIdx.x, + gridDim.x, ...
//   - once per workgroup: the single-set weight blob (wt.kblob, 59 KB) is copied into LDS.  From then on every weight is a wave-uniform
//     128-bit LDS read (ds_read_b128, all lanes one address: a broadcast) that feeds the value chain AND the net's tangent chains — 2-4 FMAs
//     per lane per weight — instead of the scalar weight stream of the step kernels' generated bodies (none of which are used here).
//   - phase 1: the nets split over the waves by PLAN8_LIN (balanced by parameters x (1 + inputs)); each lane writes value and input
//     derivatives (per degree / per unit of el) of its wave's nets to its LDS column: 42 + 68 = 110 floats per row.  The serial fp64 chains
//     of the state (sin / cos of alpha, beta, theta, phi, psi, tan theta, the atmosphere power) are computed once per tile by three of the
//     lighter waves and shared through LDS, as the latency family does.
//   - one barrier.
//   - phase 2: the 14 non-trivial columns of [A | B] (alt, phi, theta, psi, vt, alpha, beta, P, Q, R | T, el, ail, rud) split over the waves,
//     two per wave (waves 0 and 7 one: wave 0 also stores xdot, wave 7 the structurally zero npos / epos columns).  Every wave reads the 110
//     numbers and pushes its directions forward through the coefficient build-up and the equations of motion, then stores 12 floats per
//     column.  The caller never clears the output.
// Matrix instructions are not used: xdot must be bit-identical to the spec's FMA chains, which an MFMA's summation order cannot give, and
// layers 20 / 10 / 5 wide with per-row ReLU masks pad badly into 16 x 16 or 32 x 32 tiles.
// The jets, the nets on them and nlplant on them are np_model_jets.h (shared with the rollout's reverse sweep, np_model_rollout_vjp.hip).
#include "np_model_jets.h"

namespace npf16 {

typedef const LinearizeArgs __attribute__((address_space(4))) *LinArgsC;

// built for two waves per SIMD: one eight-wave workgroup per CU (the blob and the columns take 88 KB of its LDS)
__global__ __launch_bounds__(LIN_TILE * LIN_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_linearize_kernel(const LinearizeArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LIN_LDS_FLOATS];
    float *blob = lds;
    const int t = (int)(threadIdx.x % LIN_TILE);
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / LIN_TILE));
    float *col = lds + KBLOB_FLOATS + t;                   // this lane's columns, stride LIN_TILE
    float *shr = col + LIN_COLS * LIN_TILE;                // the tile's shared scalars, this lane's row

    {  // the weight blob, once per workgroup: 16 bytes per thread and turn
        typedef const f32x4 __attribute__((address_space(1))) *gv4;
        const gv4 src = (gv4)(unsigned long long)a.kblob;
        f32x4 *dst = (f32x4 *)blob;
        for (int k = (int)threadIdx.x; k < KBLOB_FLOATS / 4; k += LIN_TILE * LIN_WAVES) dst[k] = src[k];
    }

    static_assert(2 * (LIN_WAVES - 1) - 1 == NUM_LIN_DIRS - 1, "two directions per wave, one for the first and the last");
    // The loop reads the launch's arguments through the kernel-argument segment, behind an opaque statement per tile and phase
    // (NP_REREAD_ARGS, as the step kernels do): scalar loads where a value is needed.  Taken from the by-value argument instead, all of it
    // is loop-invariant and is kept in registers across both phases: 237 VGPRs and 150 SGPRs spilled to lanes, against 220 and none.
    LinArgsC ap = (LinArgsC)__builtin_amdgcn_kernarg_segment_ptr();

    const long long tiles = (a.rows + LIN_TILE - 1) / LIN_TILE;
#pragma nounroll
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        NP_REREAD_ARGS(ap);
        const long long i = tile * LIN_TILE + t;
        const bool valid = i < ap->rows;
        const unsigned r4 = (unsigned)(valid ? i : ap->rows - 1) * 4u;  // tail lanes shadow the last row; their stores are masked
        const float r2d = (float)(180.0 / 3.141592653589793);
        bool ok;
        {
            const float alpha = at_off(ap->s0 + 7 * ap->ld0, r4) * r2d, beta = at_off(ap->s0 + 8 * ap->ld0, r4) * r2d, el = at_off(ap->u0 + ap->ld0, r4);
            const float chk = ((alpha - alpha) + (beta - beta)) + (el - el);  // non-finite inputs poison every coefficient (numerics spec)
            ok = (chk == chk);

            __syncthreads();  // the blob is in LDS (first tile); every wave has read the previous tile's columns (later ones)

            // ---- phase 1 (the state is read again in phase 2: nothing but `ok` and the row's offset lives across the nets) ----
            float xn[NUM_NORM_GROUPS];
#pragma unroll
            for (int gi = 0; gi < NUM_NORM_GROUPS; gi++) {
                const float v = (gi <= G_A_RUD) ? alpha : (gi <= G_B_O ? beta : el);
                const float *h = blob + KBLOB_NORM_STRIDE * gi;  // (mean, sigma, RN(1 / sigma))
                xn[gi] = np_divc(v - h[0], h[1], h[2]);
            }
            auto state = [&](int k) { return at_off(ap->s0 + k * ap->ld0, r4); };
            // the chain below has a twin, np_model_jets.h::lin_phase1 (the reverse sweep's): which wave writes which shared scalar must stay the same in both
            if (pw == 0) {  // the lightest slice of the plan also takes theta, phi and the atmosphere power
                float a_, b_, c_;
                np_sincostan(state(4), a_, b_, c_);
                shr[4 * LIN_TILE] = a_;
                shr[5 * LIN_TILE] = b_;
                shr[8 * LIN_TILE] = c_;
                np_sincos(state(3), a_, b_);
                shr[6 * LIN_TILE] = a_;
                shr[7 * LIN_TILE] = b_;
                shr[11 * LIN_TILE] = atmos_pow(ap->af, state(2));
                eval_plan_jet<0>(blob, xn, col);
            } else if (pw == 1) {
                eval_plan_jet<1>(blob, xn, col);
            } else if (pw == 2) {
                float a_, b_;
                np_sincos(state(5), a_, b_);
                shr[9 * LIN_TILE] = a_;
                shr[10 * LIN_TILE] = b_;
                eval_plan_jet<2>(blob, xn, col);
            } else if (pw == 3) {
                eval_plan_jet<3>(blob, xn, col);
            } else if (pw == 4) {
                eval_plan_jet<4>(blob, xn, col);
            } else if (pw == 5) {
                float a_, b_;
                np_sincos(state(7), a_, b_);
                shr[0 * LIN_TILE] = a_;
                shr[1 * LIN_TILE] = b_;
                np_sincos(state(8), a_, b_);
                shr[2 * LIN_TILE] = a_;
                shr[3 * LIN_TILE] = b_;
                eval_plan_jet<5>(blob, xn, col);
            } else if (pw == 6) {
                eval_plan_jet<6>(blob, xn, col);
            } else {
                eval_plan_jet<7>(blob, xn, col);
            }
        }

        __syncthreads();  // all 110 columns and the 12 shared scalars of the tile are complete

        // ---- phase 2 ----
        NP_REREAD_ARGS(ap);
        // this wave's directions: wave 0 the first (and xdot), waves 1..6 two each, wave 7 the last (and the zero columns)
        const int dir[2] = {pw == 0 ? 0 : 2 * pw - 1, (pw == 0 || pw == LIN_WAVES - 1) ? -1 : 2 * pw};
        float s[12], u[4];
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] = at_off(ap->s0 + k * ap->ld0, r4);
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = at_off(ap->u0 + k * ap->ld0, r4);
        Jet<2> xd[12];
        nlplant_jets<2>(ap->af, s, u, shr, col, dir, ok, xd);
        if (valid) {
            const float qnan = __builtin_nanf("");
            if (pw == 0 && ap->xdot) {
#pragma unroll
                for (int k = 0; k < 12; k++) at_off(ap->xdot + k * ap->ld_out, r4) = xd[k].v;
            }
#pragma unroll
            for (int n = 0; n < 2; n++) {
                if (dir[n] < 0) continue;  // wave-uniform
                // direction d < 10 is column d + 2 of A (planes i * 12 + j), the others column d - 10 of B (planes i * 4 + j)
                const bool in_a = dir[n] < D_T;
                float *base = in_a ? ap->A + (long long)(dir[n] + 2) * ap->ld_out : ap->B + (long long)(dir[n] - D_T) * ap->ld_out;
                const long long plane = (in_a ? 12 : 4) * ap->ld_out;
#pragma unroll
                for (int k = 0; k < 12; k++) at_off(base + k * plane, r4) = (ok || k < 6) ? xd[k].d[n] : qnan;  // a non-finite alpha, beta or el: rows 6..11 are NaN, as xdot's are
            }
            if (pw == LIN_WAVES - 1) {  // nothing depends on npos and epos
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    at_off(ap->A + (long long)(k * 12) * ap->ld_out, r4) = (ok || k < 6) ? 0.0f : qnan;
                    at_off(ap->A + (long long)(k * 12 + 1) * ap->ld_out, r4) = (ok || k < 6) ? 0.0f : qnan;
                }
            }
        }
    }
}

hipError_t launch_model_linearize(int groups, const LinearizeArgs &args, hipStream_t stream) {
    if (groups < 1 || args.rows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f16_linearize_kernel, dim3((unsigned)groups), dim3(LIN_TILE * LIN_WAVES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace npf16
