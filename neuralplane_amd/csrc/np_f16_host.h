// np_f16_host.h — the host-only logic behind the C ABI (include/neuralplane_amd.h): the weights blob parsed into the three record layouts of
// np_nets.h, np_f16_airframe / np_f16_cfg / np_f16_combat_cfg rounded into the constants the kernels read (np_f16_types.h), the dispatch plan.
// These functions decide every bit the kernels compute.  No HIP in here and no library state: they run in CPU tests under host sanitizers
// (tests/host_logic_main.cpp); a function that can fail hands back its message, which np_f16_kernels.hip passes to np_last_error() unchanged.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/neuralplane_amd.h"
#include "np_dispatch.h"
#include "np_f16_types.h"
#include "np_nets.h"

namespace npf16 {

#pragma pack(push, 1)
struct BlobRec {  // NPF16MLP v1 record (tools/export_weights.py)
    char name[24];
    uint32_t input_mask, n_linear;
    uint32_t dims[6];
    double in_mean[3], in_std[3];
    double out_mean, out_std;
    uint32_t param_offset, n_params;
};
#pragma pack(pop)
static_assert(sizeof(BlobRec) == 128, "blob record is 128 bytes");

struct PackedWeights {
    std::vector<float> kb, kbd, kbg;       // the records in the first, the two-set and the GEMM-order layout (np_nets.h)
    std::vector<float> pwl, pwl_unnorm;    // blob v2: the PWL tables and their (out_std, out_mean) pairs; empty for a v1 blob
};

// Where a Linear layer in -> out keeps bias[j] and W[j][k] inside its stretch of a record, and how long that stretch is, in each record
// layout of np_nets.h (`last`: the output layer in -> 1).  The records hold the same values; only these places differ.
struct RecordLayout {
    int (*base)(int cl), (*stride)(int cl);
    int (*bias)(int in, int out, bool last, int j);
    int (*weight)(int in, int out, bool last, int j, int k);
    int (*len)(int in, int out, bool last);
};
inline const RecordLayout RECORD_LAYOUTS[3] = {
    // first: bias row, then the rows W[.][k], rows padded to even; output layer (bias, 0), W[0][.] padded to even
    {class_base, class_stride,
     [](int, int, bool, int j) { return j; },
     [](int, int out, bool last, int j, int k) { return last ? 2 + k : pad2(out) * (k + 1) + j; },
     [](int in, int out, bool last) { return last ? 2 + pad2(in) : pad2(out) * (in + 1); }},
    // two-set: (W[j][0], bias[j]) pairs, then the rows W[.][k] for k >= 1 unpadded, the layer padded to even; the output layer is such a layer
    {dual_class_base, dual_class_stride,
     [](int, int, bool, int j) { return 2 * j + 1; },
     [](int, int out, bool, int j, int k) { return k == 0 ? 2 * j : out * (k + 1) + j; },
     [](int in, int out, bool) { return pad2(out * (in + 1)); }},
    // GEMM order: as the first with the bias row behind the weight rows; output layer W[0][.] padded to even, then (bias, 0)
    {gemm_class_base, gemm_class_stride,
     [](int in, int out, bool last, int j) { return last ? pad2(in) : pad2(out) * in + j; },
     [](int, int out, bool last, int j, int k) { return last ? k : pad2(out) * k + j; },
     [](int in, int out, bool last) { return last ? pad2(in) + 2 : pad2(out) * (in + 1); }},
};

// asset blob (torch layout W[out][in]) -> kernel-order blobs (np_nets.h).  false: `err` says why the blob was refused
inline bool pack_kblob(const void *blob, size_t nbytes, PackedWeights &pw, std::string &err) {
    auto fail = [&err](const std::string &msg) {
        err = msg;
        return false;
    };
    const unsigned char *p = (const unsigned char *)blob;
    if (!p || nbytes < 16 || std::memcmp(p, "NPF16MLP", 8) != 0) return fail("weights blob: bad magic");
    uint32_t ver, nn;
    std::memcpy(&ver, p + 8, 4);
    std::memcpy(&nn, p + 12, 4);
    if ((ver != 1 && ver != 2) || nn != NUM_NETS) return fail("weights blob: unsupported version / net count");
    const size_t hdr = 16 + (size_t)nn * sizeof(BlobRec);
    if (nbytes < hdr) return fail("weights blob: truncated header");
    auto record = [p](size_t net) {
        BlobRec r;
        std::memcpy(&r, p + 16 + net * sizeof(BlobRec), sizeof(r));
        return r;
    };
    const size_t pfloats = (nbytes - hdr) / 4;
    std::vector<float> par(pfloats);
    if (pfloats) std::memcpy(par.data(), p + hdr, pfloats * 4);   // (an empty vector's data() may be null: not an argument of memcpy)
    std::vector<float> *const recs[3] = {&pw.kb, &pw.kbd, &pw.kbg};
    pw.kb.assign(KBLOB_FLOATS, 0.0f);
    pw.kbd.assign(KBLOB_DUAL_FLOATS, 0.0f);
    pw.kbg.assign(KBLOB_GEMM_FLOATS, 0.0f);
    std::vector<float> &kb = pw.kb;
    bool grp_set[NUM_NORM_GROUPS] = {};
    for (int cl = 0; cl < NUM_CLASSES; cl++) {
        const NetClass c = CLASSES[cl];
        const int hid[3] = {c.h1, c.h2, c.h3};
        const int n_hidden = c.h3 > 0 ? 3 : 2;
        for (int m = 0; m < c.count; m++) {
            const BlobRec r = record((size_t)c.nets[m]);
            const std::string nm(r.name, strnlen(r.name, sizeof(r.name)));
            if ((int)r.n_linear != n_hidden + 1 || (int)r.dims[0] != c.n_in) return fail("weights blob: shape of net " + nm + " does not match its class");
            for (int l = 0; l < n_hidden; l++)
                if ((int)r.dims[l + 1] != hid[l]) return fail("weights blob: hidden widths of net " + nm + " do not match its class");
            if ((int)r.n_params != class_params(c)) return fail("weights blob: parameter count of net " + nm);
            if ((size_t)r.param_offset + r.n_params > pfloats) return fail("weights blob: truncated parameters");
            // input slot k of the net <- k-th set bit of input_mask (bit0 alpha, bit1 beta, bit2 el)
            int slot = 0;
            for (int k = 0; k < 3; k++) {
                if (!(r.input_mask & (1u << k))) continue;
                if (slot >= c.n_in) return fail("weights blob: input mask of net " + nm);
                const int g = c.grp[slot++];
                const bool kind_ok = (k == 0 && g >= G_A_C && g <= G_A_RUD) || (k == 1 && (g == G_B_C || g == G_B_O)) ||
                                     (k == 2 && (g == G_E_C || g == G_E_ETA));
                if (!kind_ok) return fail("weights blob: input kind of net " + nm + " does not match its class");
                const float mean = (float)r.in_mean[k], sd = (float)r.in_std[k];  // torch rounds the CSV doubles to fp32
                if (!grp_set[g]) {
                    kb[KBLOB_NORM_STRIDE * g] = mean;
                    kb[KBLOB_NORM_STRIDE * g + 1] = sd;
                    kb[KBLOB_NORM_STRIDE * g + 2] = (float)(1.0 / (double)sd);  // np_divc: the normalisation divides by a per-context constant
                    grp_set[g] = true;
                } else if (kb[KBLOB_NORM_STRIDE * g] != mean || kb[KBLOB_NORM_STRIDE * g + 1] != sd) {
                    return fail("weights blob: normalisation of net " + nm + " differs from its class");
                }
            }
            if (slot != c.n_in) return fail("weights blob: input mask of net " + nm);
            // Hidden activations are carried divided by 2^ACT_SHIFT (np_nets.h): the ReLU is then the `clamp` output modifier
            // of the layer's last FMA, which costs no instruction.  Powers of two commute with every rounding, so the first
            // layer's weights and all hidden biases are stored x 2^-ACT_SHIFT and the output layer's weights x 2^+ACT_SHIFT —
            // checked here to be exact (normal, finite) for every parameter of the asset.
            bool exact = true;
            auto scaled = [&exact](float w, int e) {   // e == 0: the parameter as it is
                if (e == 0) return w;
                const float v = std::ldexp(w, e);
                if (w != 0.0f && !(std::isnormal(v) && std::ldexp(v, -e) == w)) exact = false;
                return v;
            };
            // every parameter goes to its place in each of the three records of the net; what a layout leaves unwritten is zero padding
            float *dst[3];
            for (int t = 0; t < 3; t++) dst[t] = recs[t]->data() + RECORD_LAYOUTS[t].base(cl) + (size_t)m * RECORD_LAYOUTS[t].stride(cl);
            const float *src = par.data() + r.param_offset;
            int in = c.n_in;
            for (int l = 0; l <= n_hidden; l++) {
                const bool last = l == n_hidden;
                const int out = last ? 1 : hid[l];
                const float *W = src, *bias = src + (size_t)in * out;
                for (int j = 0; j < out; j++) {
                    const float b = scaled(bias[j], last ? 0 : -ACT_SHIFT);
                    for (int t = 0; t < 3; t++) dst[t][RECORD_LAYOUTS[t].bias(in, out, last, j)] = b;
                    for (int k = 0; k < in; k++) {
                        const float w = scaled(W[j * in + k], l == 0 ? -ACT_SHIFT : last ? ACT_SHIFT : 0);
                        for (int t = 0; t < 3; t++) dst[t][RECORD_LAYOUTS[t].weight(in, out, last, j, k)] = w;
                    }
                }
                src += (size_t)in * out + out;
                for (int t = 0; t < 3; t++) dst[t] += RECORD_LAYOUTS[t].len(in, out, last);
                in = out;
            }
            if (!exact) return fail("weights blob: a parameter of net " + nm + " cannot be rescaled by 2^ACT_SHIFT exactly");
            for (int t = 0; t < 3; t++) {
                dst[t][0] = (float)r.out_std;
                dst[t][1] = (float)r.out_mean;
            }
        }
    }
    for (int g = 0; g < NUM_NORM_GROUPS; g++)
        if (!grp_set[g]) return fail("weights blob: a normalisation group is unused");
    std::copy(kb.begin(), kb.begin() + KBLOB_HEADER, pw.kbg.begin());   // the GEMM-order records sit behind the same header; the two-set ones have none
    // PWL section (blob v2): "PWL1", n_tables, seg_cap, then {net_index, n_segments, t[64], a[64], x0[64], c[64]}
    pw.pwl.clear();
    pw.pwl_unnorm.clear();
    if (ver >= 2) {
        size_t n_par = 0;
        for (int i = 0; i < NUM_NETS; i++) {
            const BlobRec r = record((size_t)i);
            n_par = std::max(n_par, (size_t)r.param_offset + r.n_params);
        }
        // offsets, not pointers: the dead net's record is checked nowhere above, its parameters may claim to end anywhere
        size_t q = hdr + n_par * 4;
        uint32_t nt, cap;
        if (q + 12 > nbytes || std::memcmp(p + q, "PWL1", 4) != 0) return fail("weights blob: PWL section missing");
        std::memcpy(&nt, p + q + 4, 4);
        std::memcpy(&cap, p + q + 8, 4);
        if (nt != NUM_PWL_TABLES || cap != PWL_SEG) return fail("weights blob: PWL section shape");
        q += 12;
        pw.pwl.assign((size_t)NUM_PWL_TABLES * PWL_TABLE_FLOATS, 0.0f);
        pw.pwl_unnorm.assign((size_t)NUM_PWL_TABLES * 2, 0.0f);
        for (uint32_t k = 0; k < nt; k++) {
            uint32_t idx, nseg;
            if (q + 8 + PWL_TABLE_FLOATS * 4 > nbytes) return fail("weights blob: truncated PWL section");
            std::memcpy(&idx, p + q, 4);
            std::memcpy(&nseg, p + q + 4, 4);
            if (idx >= (uint32_t)NUM_NETS || pwl_index((int)idx) != (int)k || nseg < 1 || nseg > (uint32_t)PWL_SEG)
                return fail("weights blob: PWL table order does not match the kernel's");
            std::memcpy(pw.pwl.data() + (size_t)k * PWL_TABLE_FLOATS, p + q + 8, PWL_TABLE_FLOATS * 4);
            const BlobRec r = record(idx);
            pw.pwl_unnorm[2 * k] = (float)r.out_std;
            pw.pwl_unnorm[2 * k + 1] = (float)r.out_mean;
            q += 8 + PWL_TABLE_FLOATS * 4;
        }
    }
    return true;
}

// np_f16_airframe -> the fp32 constants of the kernels.  Every value is rounded where the literal expression of the reference rounds it:
// plain literals are Python doubles that enter fp32 tensor arithmetic (one rounding), derived constants are folded in double first
// (F16_dynamics.py:221-227 evaluates e.g. Jz * (Jz - Jy) + Jxz ** 2 in Python before it meets a tensor).
inline np_f16_airframe airframe_defaults() {
    np_f16_airframe a = {};
    a.g = 32.17; a.mass = 636.94; a.B = 30.0; a.S = 300.0; a.cbar = 11.32; a.xcgr = 0.35; a.xcg = 0.30; a.Heng = 0.0;
    a.Jy = 55814.0; a.Jxz = 982.0; a.Jz = 63100.0; a.Jx = 9496.0;
    a.ail_ref = 21.5; a.rud_ref = 30.0;
    a.atm_lapse = 0.703e-5; a.atm_exp = 4.14; a.rho0 = 2.377e-3;
    a.lag_keep = 0.9; a.lag_new = 0.1; a.thrust_frac = 0.225; a.thrust_max = 76300.0; a.thrust_unit = 0.3048;
    a.surf_max[0] = a.surf_max[1] = a.surf_max[2] = 45.0;
    return a;
}

inline bool airframe_is_zero(const np_f16_airframe &a) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&a);
    for (size_t k = 0; k < sizeof(a); k++)
        if (p[k]) return false;
    return true;
}

inline const char *airframe_error(const np_f16_airframe &a) {
    const double pos[] = {a.mass, a.B, a.S, a.cbar, a.Jy, a.Jz, a.Jx, a.ail_ref, a.rud_ref, a.rho0, a.thrust_unit, a.atm_exp};
    for (double v : pos)
        if (!(v > 0.0) || !std::isfinite(v)) return "airframe: mass, B, S, cbar, Jx, Jy, Jz, ail_ref, rud_ref, rho0, thrust_unit and atm_exp must be positive and finite";
    if (!(a.Jx * a.Jz - a.Jxz * a.Jxz > 0.0)) return "airframe: Jx Jz - Jxz^2 must be positive";
    const double fin[] = {a.g, a.xcgr, a.xcg, a.Heng, a.Jxz, a.atm_lapse, a.atm_exp, a.lag_keep, a.lag_new, a.thrust_frac, a.thrust_max, a.surf_max[0], a.surf_max[1], a.surf_max[2]};
    for (double v : fin)
        if (!std::isfinite(v)) return "airframe: non-finite value";
    return nullptr;
}

inline Airframe make_airframe(const np_f16_airframe &in) {
    const np_f16_airframe a = airframe_is_zero(in) ? airframe_defaults() : in;
    auto rcp = [](float c) { return (float)(1.0 / (double)c); };   // NP_RCP_CONST: RN(1 / c) of the fp32 divisor
    Airframe d;
    d.g = (float)a.g; d.mass = (float)a.mass; d.r_mass = rcp(d.mass); d.B = (float)a.B; d.S = (float)a.S; d.cbar = (float)a.cbar; d.Heng = (float)a.Heng;
    d.Jy = (float)a.Jy; d.r_Jy = rcp(d.Jy); d.Jxz = (float)a.Jxz; d.Jz = (float)a.Jz; d.Jx = (float)a.Jx;
    d.xc = (float)(a.xcgr - a.xcg);
    d.cbar_over_B = (float)(a.cbar / a.B);
    d.c1 = (float)(a.Jz * (a.Jz - a.Jy) + a.Jxz * a.Jxz);
    d.c2 = (float)(a.Jxz * (a.Jx - a.Jy + a.Jz));
    d.c3 = (float)(a.Jz - a.Jx);
    d.c4 = (float)(a.Jx * (a.Jx - a.Jy) + a.Jxz * a.Jxz);
    d.denom = (float)(a.Jx * a.Jz - a.Jxz * a.Jxz);
    d.r_denom = rcp(d.denom);
    d.ail_ref = (float)a.ail_ref; d.r_ail_ref = rcp(d.ail_ref); d.rud_ref = (float)a.rud_ref; d.r_rud_ref = rcp(d.rud_ref);
    d.atm_lapse = (float)a.atm_lapse; d.atm_exp = (double)(float)a.atm_exp; d.rho0 = (float)a.rho0; d.pad_ = 0.0f;
    d.lag_keep = (float)a.lag_keep; d.lag_new = (float)a.lag_new; d.thrust_frac = (float)a.thrust_frac; d.thrust_max = (float)a.thrust_max;
    d.thrust_unit = (float)a.thrust_unit; d.r_thrust_unit = rcp(d.thrust_unit);
    for (int k = 0; k < 3; k++) d.surf_max[k] = (float)a.surf_max[k];
    return d;
}

// ---- fleets (np_f16_set_fleet): per-row airframes ---------------------------------------------------------------------------------
// One record of the device table: make_airframe's constants with the two stretches of padding inside an Airframe (before atm_exp, behind
// surf_max) zeroed, so that a table is a function of its classes byte for byte.
// Field by field: a field added to Airframe (np_f16_types.h) must be added below, or every fleet flies it as zero — the size is pinned so
// that such a change stops here first (160 bytes: 36 floats and the double atm_exp, 4 + 4 bytes of padding).
static_assert(sizeof(Airframe) == 160, "Airframe changed: copy the new field in fleet_record, then update this size");
inline Airframe fleet_record(const np_f16_airframe &c) {
    const Airframe v = make_airframe(c);
    Airframe r;
    std::memset(&r, 0, sizeof(r));
    r.g = v.g; r.mass = v.mass; r.r_mass = v.r_mass; r.B = v.B; r.S = v.S; r.cbar = v.cbar; r.Heng = v.Heng; r.pad_ = v.pad_;
    r.Jy = v.Jy; r.r_Jy = v.r_Jy; r.Jxz = v.Jxz; r.Jz = v.Jz; r.Jx = v.Jx;
    r.xc = v.xc; r.cbar_over_B = v.cbar_over_B; r.c1 = v.c1; r.c2 = v.c2; r.c3 = v.c3; r.c4 = v.c4; r.denom = v.denom; r.r_denom = v.r_denom;
    r.ail_ref = v.ail_ref; r.r_ail_ref = v.r_ail_ref; r.rud_ref = v.rud_ref; r.r_rud_ref = v.r_rud_ref;
    r.atm_lapse = v.atm_lapse; r.rho0 = v.rho0; r.atm_exp = v.atm_exp;
    r.lag_keep = v.lag_keep; r.lag_new = v.lag_new; r.thrust_frac = v.thrust_frac; r.thrust_max = v.thrust_max;
    r.thrust_unit = v.thrust_unit; r.r_thrust_unit = v.r_thrust_unit;
    for (int k = 0; k < 3; k++) r.surf_max[k] = v.surf_max[k];
    return r;
}

// The table of a fleet: record k = fleet_record(classes[k]) (an all-zero block = the F-16).  false: `err` says why — the class count, or the
// first class airframe_error refuses, by number.
inline bool fleet_table(const np_f16_airframe *classes, int64_t k, std::vector<Airframe> &out, std::string &err) {
    out.clear();
    if (k < 1 || k > FLEET_MAX_CLASSES) {
        err = "fleet: the number of airframe classes must be 1 .. " + std::to_string(FLEET_MAX_CLASSES) + " (got " + std::to_string(k) + ")";
        return false;
    }
    if (!classes) {
        err = "fleet: null class table";
        return false;
    }
    for (int64_t c = 0; c < k; c++) {
        if (airframe_is_zero(classes[c])) continue;
        if (const char *e = airframe_error(classes[c])) {
            err = "fleet: class " + std::to_string(c) + ": " + e;
            return false;
        }
    }
    out.resize((size_t)k);
    for (int64_t c = 0; c < k; c++) out[(size_t)c] = fleet_record(classes[c]);
    return true;
}

// What a context with a fleet cannot be or do: null, or the refusal (every message names the fleet).  combat / gemm_order / variant: the
// context's; the fleet kernels are the single-set throughput shape of the MLP and the table numerics.
inline const char *fleet_context_error(bool combat, bool gemm_order, int variant) {
    if (combat) return "fleet: SingleCombat contexts have no fleet kernels (one airframe per context: np_f16_combat_cfg.airframe)";
    if (gemm_order) return "fleet: a context with aero_gemm_order has no fleet kernels (the fleet kernels are built for the default order of the aero nets)";
    if (variant != NP_KERNEL_AUTO && variant != NP_KERNEL_THROUGHPUT)
        return "fleet: a context with a fleet runs the throughput-shaped fleet kernel at every n (np_f16_set_kernel_variant: NP_KERNEL_AUTO or NP_KERNEL_THROUGHPUT only)";
    return nullptr;
}
// np_planning_inner_loop on a context with a fleet: launch by launch only
inline const char *fleet_planning_error(int mode) {
    if (mode >= NP_PLANNING_PERSISTENT)
        return "np_planning_loop: a context with a fleet runs launch by launch (the persistent kernel and its guest / queue / dual schedules read one airframe per context); mode must be NP_PLANNING_AUTO or NP_PLANNING_LAUNCHES";
    return nullptr;
}
// a launch of `n` rows starting at row `off` of the index np_f16_set_fleet_index registered for `index_n` rows
inline const char *fleet_launch_error(bool have_index, int64_t index_n, int64_t off, int64_t n) {
    if (!have_index) return "fleet: no airframe index (np_f16_set_fleet_index) for a context with a fleet";
    if (off < 0 || off + n > index_n) return "fleet: the launch covers more rows than the airframe index registered with np_f16_set_fleet_index";
    return nullptr;
}

inline DevCfg make_devcfg(const np_f16_cfg &c) {
    DevCfg d;
    d.af = make_airframe(c.airframe);
    d.dt = (float)c.dt - 0.0f;  // t = tensor([0., dt]); dt = t1 - t0   (F16_model.py:66)
    d.airspeed = (float)c.airspeed;
    d.noise_scale = (float)c.noise_scale;
    d.altitude_limit = (float)c.altitude_limit;
    d.acceleration_limit = (float)c.acceleration_limit;
    d.max_velocity = (float)c.max_velocity;
    d.min_velocity = (float)c.min_velocity;
    d.min_alpha = (float)c.min_alpha;
    d.max_alpha = (float)c.max_alpha;
    d.min_beta = (float)c.min_beta;
    d.max_beta = (float)c.max_beta;
    d.max_check_interval = c.max_check_interval;
    d.min_check_interval = c.min_check_interval;
    d.init_T = (float)c.init_T;
    d.alt_span = (float)(c.max_altitude - c.min_altitude);  // Python arithmetic first, then one rounding
    d.min_altitude = (float)c.min_altitude;
    d.vt_span = (float)(c.max_vt - c.min_vt);
    d.min_vt = (float)c.min_vt;
    d.max_heading_increment = (float)c.max_heading_increment;
    d.max_pitch_increment = (float)c.max_pitch_increment;
    d.max_velocities_u_increment = (float)c.max_velocities_u_increment;
    d.dist_span = (float)(c.max_distance - c.min_distance);
    d.min_distance = (float)c.min_distance;
    d.aero_1d_tables = c.aero_1d_tables ? 1 : 0;
    return d;
}

inline PidDev make_pid(const np_pid_gains &g, double dt) {
    PidDev p;
    p.Kp = (float)g.Kp;
    p.Ki = (float)g.Ki;
    p.Kd = (float)g.Kd;
    p.Kff = (float)g.Kff;
    p.Kimax = (float)g.Kimax;
    p.tau = (float)(g.tau < 0.05 ? 0.05 : g.tau);  // rollController.py:44-45
    p.rmax_pos = (float)g.rmax_pos;
    p.rmax_neg = (float)g.rmax_neg;
    p.ki_on = (g.Ki != 0.0 && dt > 0.0) ? 1 : 0;
    return p;
}

inline CombatDevCfg make_combat_devcfg(const np_f16_combat_cfg &c) {
    CombatDevCfg d;
    d.af = make_airframe(c.airframe);
    d.dt = (float)c.dt - 0.0f;
    d.dt_pid = (float)c.dt;
    d.airspeed = (float)c.airspeed;
    d.altitude_limit = (float)c.altitude_limit;
    d.acceleration_limit = (float)c.acceleration_limit;
    d.max_velocity = (float)c.max_velocity;
    d.min_velocity = (float)c.min_velocity;
    d.min_alpha = (float)c.min_alpha;
    d.max_alpha = (float)c.max_alpha;
    d.min_beta = (float)c.min_beta;
    d.max_beta = (float)c.max_beta;
    d.dist_limit_sq = (float)(c.distance_limit * c.distance_limit);  // `self.distance_limit ** 2` is Python arithmetic
    d.max_steps = c.max_steps;
    d.init_T = (float)c.init_T;
    d.alt_span = (float)(c.max_altitude - c.min_altitude);
    d.min_altitude = (float)c.min_altitude;
    d.vt_span = (float)(c.max_vt - c.min_vt);
    d.min_vt = (float)c.min_vt;
    d.yaw_span = (float)(c.max_heading - c.min_heading);
    d.min_heading = (float)c.min_heading;
    d.npos_span = (float)(c.max_npos - c.min_npos);
    d.min_npos = (float)c.min_npos;
    d.epos_span = (float)(c.max_epos - c.min_epos);
    d.min_epos = (float)c.min_epos;
    d.roll = make_pid(c.roll, c.dt);
    d.pitch = make_pid(c.pitch, c.dt);
    d.yaw = make_pid(c.yaw, c.dt);
    d.roll_ff = (float)c.roll_ff;
    d.gravity = (float)c.gravity;
    d.scale_min = (float)std::min(0.5, 1000.0 / (2.0 * c.airspeed_max));   // controller.py:36-37
    d.scale_max = (float)std::max(2.0, 1000.0 / (0.7 * c.airspeed_min));
    d.inner_steps = c.inner_steps;
    d.aero_1d_tables = c.aero_1d_tables ? 1 : 0;
    return d;
}

// np_dispatch_plan / np_dispatch_plan_gemm (`gemm`): null, or why the arguments were refused.  block: the env kernels' NPF16_BLOCK
inline const char *dispatch_plan(int64_t n, int32_t num_cus, int32_t step, int32_t solver, int32_t tables, int32_t gemm, int32_t variant, int block,
                                 np_dispatch_info *out) {
    if (!out) return "null argument";
    if (n <= 0 || num_cus <= 0) return "np_dispatch_plan: n and num_cus must be positive";
    if (variant < NP_KERNEL_AUTO || variant > NP_KERNEL_DUAL4) return "np_dispatch_plan: unknown variant";
    const bool dual_pin = variant == NP_KERNEL_DUAL8 || variant == NP_KERNEL_DUAL4;   // SingleCombat only: the env kernels keep their size rule
    const npdispatch::EnvChoice c = npdispatch::env_choice(n, num_cus, step != 0, solver, tables != 0, dual_pin ? NP_KERNEL_AUTO : variant, NP_KERNEL_AUTO, 0, block, gemm != 0);
    const npdispatch::Limits l = npdispatch::limits_for(num_cus);
    out->pair = c.pair; out->pair3 = c.pair3; out->latency = c.latency; out->latency8 = c.latency8; out->latency2 = c.latency2;
    out->latency4w = c.latency4w; out->block = c.block; out->grid = c.grid;
    out->planning_groups = npdispatch::planning_groups(n, num_cus);
    out->actor_tile32 = npdispatch::actor_tile32(n, num_cus) ? 1 : 0;
    const int dual = !(step && solver == 0 && !tables) ? 0 : dual_pin ? (variant == NP_KERNEL_DUAL8 ? 8 : 4)
                     : variant == NP_KERNEL_AUTO ? npdispatch::combat_dual_waves(n, num_cus) : 0;
    out->combat_latency = dual == 8 ? 2 : dual == 4 ? 3 : n <= l.combat_lat_max_n ? 1 : 0;
    out->planning_mode = gemm ? (int)npdispatch::PL_LAUNCHES : npdispatch::planning_mode(n, num_cus);   // one eight-wave workgroup per CU
    out->planning_mode_i8 = gemm ? (int)npdispatch::PL_LAUNCHES : npdispatch::planning_mode(n, num_cus, true);
    return nullptr;
}

}  // namespace npf16
