// fleet_host_main.cpp — the host logic of a fleet (per-row airframes: neuralplane_amd/csrc/np_f16_host.h::fleet_table and the refusals beside it)
// as a stand-alone program, for tests/test_fleet_cpu.py: built with g++ and the host sanitizers, no HIP and no library.
//
//     fleet_host_main
//
// Checks, each with a line on stdout (`ok <what>`); the first check that fails prints `FAIL <what>` on stderr and ends the program with status 1:
//   the table of K classes equals K separate fleet_record results byte for byte, and each of those holds make_airframe's constants
//   (every field; the two stretches of padding inside an Airframe are zero); an all-zero class is the F-16; K = 0 and K = 65 537 are
//   refused; a non-finite mass in class 2 is refused with "class 2" in the message; the context / planning / launch refusals name the fleet.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../neuralplane_amd/csrc/np_f16_host.h"

using namespace npf16;

static void check(bool ok, const char *what) {
    if (!ok) {
        std::fprintf(stderr, "FAIL %s\n", what);
        std::exit(1);
    }
    std::printf("ok %s\n", what);
}

// the bytes of an Airframe that hold a value: everything but the padding in front of atm_exp and behind surf_max
static bool same_values(const Airframe &a, const Airframe &b) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&a), *q = reinterpret_cast<const unsigned char *>(&b);
    const size_t end0 = offsetof(Airframe, rho0) + sizeof(float), beg1 = offsetof(Airframe, atm_exp), end1 = offsetof(Airframe, surf_max) + 3 * sizeof(float);
    return std::memcmp(p, q, end0) == 0 && std::memcmp(p + beg1, q + beg1, end1 - beg1) == 0;
}
static bool padding_is_zero(const Airframe &a) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&a);
    const size_t end0 = offsetof(Airframe, rho0) + sizeof(float), beg1 = offsetof(Airframe, atm_exp), end1 = offsetof(Airframe, surf_max) + 3 * sizeof(float);
    for (size_t k = end0; k < beg1; k++)
        if (p[k]) return false;
    for (size_t k = end1; k < sizeof(Airframe); k++)
        if (p[k]) return false;
    return true;
}

int main() {
    static_assert(sizeof(Airframe) % 16 == 0, "the kernels load a record as 16-byte vectors");
    // five classes: the F-16 as the all-zero block, the F-16 spelled out, and three that move mass / inertia, geometry and c.g., thrust and atmosphere
    std::vector<np_f16_airframe> cls(5);
    cls[0] = np_f16_airframe{};
    cls[1] = airframe_defaults();
    cls[2] = airframe_defaults();
    cls[2].mass = 700.0;
    cls[2].Jy = 60000.0;
    cls[3] = airframe_defaults();
    cls[3].xcg = 0.25;
    cls[3].S = 320.0;
    cls[3].Jxz = 1100.0;
    cls[4] = airframe_defaults();
    cls[4].thrust_max = 60000.0;
    cls[4].atm_lapse = 0.65e-5;
    cls[4].atm_exp = 4.3;
    cls[4].surf_max[1] = 30.0;

    std::vector<Airframe> table;
    std::string err;
    check(fleet_table(cls.data(), (int64_t)cls.size(), table, err) && err.empty(), "five classes are accepted");
    check(table.size() == cls.size(), "one record per class");
    bool bytes_equal = true, values_equal = true, pad_zero = true;
    for (size_t k = 0; k < cls.size(); k++) {
        const Airframe one = fleet_record(cls[k]), made = make_airframe(cls[k]);
        bytes_equal = bytes_equal && std::memcmp(&table[k], &one, sizeof(Airframe)) == 0;
        values_equal = values_equal && same_values(table[k], made);
        pad_zero = pad_zero && padding_is_zero(table[k]);
    }
    check(bytes_equal, "K records equal K separate results byte for byte");
    check(values_equal, "every record holds make_airframe's constants of its class");
    check(pad_zero, "the padding of every record is zero");
    check(std::memcmp(&table[0], &table[1], sizeof(Airframe)) == 0, "the all-zero class is the F-16");
    check(std::memcmp(&table[0], &table[2], sizeof(Airframe)) != 0 && table[2].mass == 700.0f && table[2].r_mass == (float)(1.0 / (double)700.0f),
          "a class that differs gives a record that differs, reciprocal included");
    // a single class, and the largest table
    check(fleet_table(&cls[2], 1, table, err) && table.size() == 1 && std::memcmp(&table[0], &(const Airframe &)fleet_record(cls[2]), sizeof(Airframe)) == 0, "K = 1");
    {
        std::vector<np_f16_airframe> big((size_t)FLEET_MAX_CLASSES, np_f16_airframe{});
        big.back() = cls[4];
        check(fleet_table(big.data(), FLEET_MAX_CLASSES, table, err) && table.size() == (size_t)FLEET_MAX_CLASSES && same_values(table.back(), make_airframe(cls[4])),
              "K = 65536 is accepted");
        big.push_back(np_f16_airframe{});
        err.clear();
        check(!fleet_table(big.data(), FLEET_MAX_CLASSES + 1, table, err) && table.empty() && err.find("fleet") != std::string::npos, "K = 65537 is refused");
    }
    err.clear();
    check(!fleet_table(cls.data(), 0, table, err) && table.empty() && err.find("fleet") != std::string::npos, "K = 0 is refused");
    err.clear();
    check(!fleet_table(cls.data(), -3, table, err) && !err.empty(), "a negative K is refused");
    err.clear();
    check(!fleet_table(nullptr, 2, table, err) && !err.empty(), "a null class table is refused");
    {
        std::vector<np_f16_airframe> bad = cls;
        bad[2].mass = std::numeric_limits<double>::infinity();
        err.clear();
        check(!fleet_table(bad.data(), (int64_t)bad.size(), table, err) && table.empty() && err.find("class 2") != std::string::npos && err.find("fleet") != std::string::npos,
              "a non-finite mass in class 2 is refused by class number");
        std::printf("message %s\n", err.c_str());
        bad = cls;
        bad[4].Jy = std::nan("");
        err.clear();
        check(!fleet_table(bad.data(), (int64_t)bad.size(), table, err) && err.find("class 4") != std::string::npos, "a NaN inertia in class 4 is refused by class number");
    }
    // what a context with a fleet cannot be or do
    auto names_fleet = [](const char *e) { return e && std::string(e).find("fleet") != std::string::npos; };
    check(fleet_context_error(false, false, NP_KERNEL_AUTO) == nullptr && fleet_context_error(false, false, NP_KERNEL_THROUGHPUT) == nullptr, "auto and throughput are allowed");
    check(names_fleet(fleet_context_error(true, false, NP_KERNEL_AUTO)), "a combat context is refused");
    check(names_fleet(fleet_context_error(false, true, NP_KERNEL_AUTO)), "aero_gemm_order is refused");
    bool pins = true;
    for (int v : {NP_KERNEL_LATENCY, NP_KERNEL_PAIR, NP_KERNEL_LATENCY8, NP_KERNEL_LATENCY2, NP_KERNEL_LATENCY4W, NP_KERNEL_DUAL8, NP_KERNEL_DUAL4})
        pins = pins && names_fleet(fleet_context_error(false, false, v));
    check(pins, "every other kernel variant is refused");
    check(fleet_planning_error(NP_PLANNING_AUTO) == nullptr && fleet_planning_error(NP_PLANNING_LAUNCHES) == nullptr, "planning: auto and launches are allowed");
    bool modes = true;
    for (int m : {NP_PLANNING_PERSISTENT, NP_PLANNING_PERSISTENT_QUEUE, NP_PLANNING_PERSISTENT_GUESTS, NP_PLANNING_PERSISTENT_DUAL}) modes = modes && names_fleet(fleet_planning_error(m));
    check(modes, "planning: the persistent, queue, guest and dual modes are refused");
    check(fleet_launch_error(true, 293, 0, 293) == nullptr && fleet_launch_error(true, 293, 128, 165) == nullptr, "a launch inside the index is allowed");
    check(names_fleet(fleet_launch_error(true, 293, 0, 294)) && names_fleet(fleet_launch_error(true, 293, 256, 64)) && names_fleet(fleet_launch_error(false, 0, 0, 1)),
          "a launch beyond the index, or without one, is refused");
    return 0;
}
