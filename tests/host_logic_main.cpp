// host_logic_main.cpp — the host-only logic of the C ABI (neuralplane_amd/csrc/np_f16_host.h) as a stand-alone program, for
// tests/test_host_header_cpu.py: built with g++ and the host sanitizers, no HIP and no library.
//
//     host_logic_main BLOB OUTDIR CFG COMBAT_CFG
//
// BLOB: the NPF16MLP weights asset.  CFG / COMBAT_CFG: the raw bytes of an np_f16_cfg / np_f16_combat_cfg.
// Writes OUTDIR/{kb,kbd,kbg,pwl,pwl_unnorm}.f32 (raw fp32; the last two for a version-2 blob), re-runs the packer on cut and corrupted copies
// of the blob (each must be refused with a message; one line per case on stderr), and prints `name value-bits` lines for the Airframe of the
// default airframe block and for the DevCfg / CombatDevCfg of the two records.  Exit status 0: everything held.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "../neuralplane_amd/csrc/np_f16_host.h"

using namespace npf16;
typedef std::vector<unsigned char> Bytes;

static Bytes read_file(const char *path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void write_floats(const std::string &path, const std::vector<float> &v) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(float)));
    if (!f) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        std::exit(2);
    }
}

static int n_bad = 0;
// the packer on a heap copy of exactly `n` bytes (so that a read past the end is a sanitizer report): it must refuse, and say why
static void must_refuse(const std::string &what, const Bytes &blob, size_t n) {
    unsigned char *copy = new unsigned char[n ? n : 1];
    std::memcpy(copy, blob.data(), n);
    PackedWeights pw;
    std::string err;
    const bool ok = pack_kblob(copy, n, pw, err);
    delete[] copy;
    std::fprintf(stderr, "%-44s %s\n", what.c_str(), ok ? "ACCEPTED" : err.c_str());
    if (ok || err.empty()) n_bad++;
}
static void must_refuse_patched(const std::string &what, Bytes blob, size_t at, uint32_t value) {
    std::memcpy(blob.data() + at, &value, 4);
    must_refuse(what, blob, blob.size());
}

static void bits(const char *name, float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    std::printf("%s %08x\n", name, u);
}
static void bits(const char *name, double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    std::printf("%s %016llx\n", name, (unsigned long long)u);
}
static void bits(const char *name, long long v) { std::printf("%s %lld\n", name, v); }
static void bits(const char *name, int v) { std::printf("%s %d\n", name, v); }
#define F(rec, prefix, field) bits(prefix #field, (rec).field)

static void print_airframe(const char *prefix, const Airframe &a) {
    std::string p(prefix);
#define A(field) bits((p + #field).c_str(), a.field)
    A(g); A(mass); A(r_mass); A(B); A(S); A(cbar); A(Heng); A(pad_); A(Jy); A(r_Jy); A(Jxz); A(Jz); A(Jx); A(xc); A(cbar_over_B);
    A(c1); A(c2); A(c3); A(c4); A(denom); A(r_denom); A(ail_ref); A(r_ail_ref); A(rud_ref); A(r_rud_ref); A(atm_lapse); A(rho0); A(atm_exp);
    A(lag_keep); A(lag_new); A(thrust_frac); A(thrust_max); A(thrust_unit); A(r_thrust_unit); A(surf_max[0]); A(surf_max[1]); A(surf_max[2]);
#undef A
}
static void print_pid(const char *prefix, const PidDev &g) {
    std::string p(prefix);
#define P(field) bits((p + #field).c_str(), g.field)
    P(Kp); P(Ki); P(Kd); P(Kff); P(Kimax); P(tau); P(rmax_pos); P(rmax_neg); P(ki_on);
#undef P
}

int main(int argc, char **argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s BLOB OUTDIR CFG COMBAT_CFG\n", argv[0]);
        return 2;
    }
    const Bytes blob = read_file(argv[1]);
    const std::string dir(argv[2]);

    // ---- layouts ----
    PackedWeights pw;
    std::string err;
    if (!pack_kblob(blob.data(), blob.size(), pw, err)) {
        std::fprintf(stderr, "the asset was refused: %s\n", err.c_str());
        return 1;
    }
    write_floats(dir + "/kb.f32", pw.kb);
    write_floats(dir + "/kbd.f32", pw.kbd);
    write_floats(dir + "/kbg.f32", pw.kbg);
    uint32_t ver;
    std::memcpy(&ver, blob.data() + 8, 4);
    if (ver >= 2) {
        write_floats(dir + "/pwl.f32", pw.pwl);
        write_floats(dir + "/pwl_unnorm.f32", pw.pwl_unnorm);
    }

    // ---- hostile input ----
    const size_t rec0 = 16, rec = sizeof(BlobRec), hdr = rec0 + NUM_NETS * rec;
    size_t n_par = 0;
    for (int i = 0; i < NUM_NETS; i++) {
        BlobRec r;
        std::memcpy(&r, blob.data() + rec0 + i * rec, rec);
        n_par = std::max(n_par, (size_t)r.param_offset + r.n_params);
    }
    const size_t pwl0 = hdr + 4 * n_par;   // where the PWL section starts (version 2)
    for (size_t n : {(size_t)0, (size_t)8, (size_t)15, (size_t)16}) must_refuse("cut at " + std::to_string(n), blob, n);
    for (int i = 0; i < NUM_NETS; i++) {
        must_refuse("cut one byte short of the end of record " + std::to_string(i), blob, rec0 + (i + 1) * rec - 1);
        must_refuse("cut at the end of record " + std::to_string(i), blob, rec0 + (i + 1) * rec);
    }
    must_refuse("cut inside the parameter block", blob, hdr + 4 * (n_par / 2) + 1);
    if (ver >= 2) {
        must_refuse("cut at the start of the PWL section", blob, pwl0);
        must_refuse("cut inside the PWL section's header", blob, pwl0 + 7);
        must_refuse("cut inside the PWL tables", blob, pwl0 + 12 + 3 * (8 + 4 * PWL_TABLE_FLOATS) + 5);
        must_refuse("cut one byte short of the end of the PWL section", blob, blob.size() - 1);
    }
    const int member = N_Cxq, dead = N_dCzq_lef;   // a member of the first class; the net no class holds
    const size_t m0 = rec0 + member * rec;
    must_refuse_patched("n_linear of a class member", blob, m0 + offsetof(BlobRec, n_linear), 9);
    must_refuse_patched("dims[0] of a class member", blob, m0 + offsetof(BlobRec, dims), 2);
    must_refuse_patched("dims[1] of a class member", blob, m0 + offsetof(BlobRec, dims) + 4, 21);
    must_refuse_patched("n_params of a class member", blob, m0 + offsetof(BlobRec, n_params), 262);
    must_refuse_patched("input_mask of a class member: no input", blob, m0 + offsetof(BlobRec, input_mask), 0);
    must_refuse_patched("input_mask of a class member: wrong kind", blob, m0 + offsetof(BlobRec, input_mask), 2);
    must_refuse_patched("input_mask of a class member: too many", blob, m0 + offsetof(BlobRec, input_mask), 3);
    must_refuse_patched("param_offset of a class member", blob, m0 + offsetof(BlobRec, param_offset), 0xFFFFFFF0u);
    if (ver >= 2) {
        must_refuse_patched("param_offset of the dead net", blob, rec0 + dead * rec + offsetof(BlobRec, param_offset), 0xFFFFFFF0u);
        must_refuse_patched("PWL net_index out of range", blob, pwl0 + 12, 0xFFFFFFFFu);
        must_refuse_patched("PWL net_index of another table", blob, pwl0 + 12, (uint32_t)N_Cyr);
        must_refuse_patched("PWL net_index of a multi-input net", blob, pwl0 + 12, (uint32_t)N_Cx);
        must_refuse_patched("PWL n_segments 0", blob, pwl0 + 16, 0);
        must_refuse_patched("PWL n_segments above the cap", blob, pwl0 + 16, PWL_SEG + 1);
    }
    if (n_bad) {
        std::fprintf(stderr, "%d hostile blobs were accepted or refused without a message\n", n_bad);
        return 1;
    }

    // ---- constants ----
    if (airframe_error(airframe_defaults()) != nullptr) return 1;
    print_airframe("airframe.", make_airframe(airframe_defaults()));
    const Bytes cb = read_file(argv[3]), ccb = read_file(argv[4]);
    np_f16_cfg cfg;
    np_f16_combat_cfg ccfg;
    if (cb.size() != sizeof(cfg) || ccb.size() != sizeof(ccfg)) {
        std::fprintf(stderr, "np_f16_cfg is %zu bytes (got %zu), np_f16_combat_cfg %zu (got %zu)\n", sizeof(cfg), cb.size(), sizeof(ccfg), ccb.size());
        return 2;
    }
    std::memcpy(&cfg, cb.data(), sizeof(cfg));
    std::memcpy(&ccfg, ccb.data(), sizeof(ccfg));
    const DevCfg d = make_devcfg(cfg);
#define D(field) F(d, "devcfg.", field)
    D(dt); D(airspeed); D(noise_scale); D(altitude_limit); D(acceleration_limit); D(max_velocity); D(min_velocity); D(min_alpha); D(max_alpha);
    D(min_beta); D(max_beta); D(max_check_interval); D(min_check_interval); D(init_T); D(alt_span); D(min_altitude); D(vt_span); D(min_vt);
    D(max_heading_increment); D(max_pitch_increment); D(max_velocities_u_increment); D(dist_span); D(min_distance); D(aero_1d_tables);
#undef D
    print_airframe("devcfg.af.", d.af);
    const CombatDevCfg c = make_combat_devcfg(ccfg);
#define K(field) F(c, "combat.", field)
    K(dt); K(dt_pid); K(airspeed); K(altitude_limit); K(acceleration_limit); K(max_velocity); K(min_velocity); K(min_alpha); K(max_alpha);
    K(min_beta); K(max_beta); K(dist_limit_sq); K(max_steps); K(init_T); K(alt_span); K(min_altitude); K(vt_span); K(min_vt); K(yaw_span);
    K(min_heading); K(npos_span); K(min_npos); K(epos_span); K(min_epos); K(roll_ff); K(gravity); K(scale_min); K(scale_max); K(inner_steps);
    K(aero_1d_tables);
#undef K
    print_pid("combat.roll.", c.roll);
    print_pid("combat.pitch.", c.pitch);
    print_pid("combat.yaw.", c.yaw);
    print_airframe("combat.af.", c.af);
    return 0;
}
