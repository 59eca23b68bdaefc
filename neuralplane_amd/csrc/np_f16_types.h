// np_f16_types.h — the plain records the host builds and the kernels read as arguments: packed-weight pointers, the airframe, the scenario
// constants.  No HIP in here: np_f16_host.h fills them in CPU tests (tests/host_logic_main.cpp); the device headers include this one.
#pragma once

// Airframe::get() is device code in a HIP translation unit and an ordinary inline function anywhere else
#ifdef __HIPCC__
#define NP_DEVICE_INLINE __device__ __forceinline__
#else
#define NP_DEVICE_INLINE inline
#endif

namespace npf16 {

// The packed weights of one aircraft type (np_nets.h KBLOB layout + the optional PWL tables) live in device buffers owned
// by a context, so contexts with different weight sets (a second aircraft with the same net topology) coexist on a device.
struct AeroWeights {
    const float *kblob;       // [KBLOB_FLOATS]
    const float *kblob_dual;  // [KBLOB_DUAL_FLOATS] the same nets in the record layout of the two-set bodies (np_nets.h)
    const float *pwl;         // [NUM_PWL_TABLES * PWL_TABLE_FLOATS] or null
    const float *pwl_unnorm;  // [NUM_PWL_TABLES * 2] or null
    const float *kblob_gemm;  // [KBLOB_GEMM_FLOATS] the records of the GEMM-order bodies (np_nets.h), or null: contexts with aero_gemm_order only
};

// The airframe as data (np_f16_airframe, ABI 16): what F16Dynamics.nlplant / atmos and F16Model.update spell as literals
// (envs/models/F16/F16_dynamics.py:22-35,61-76,114-116; envs/models/F16_model.py:52-62), rounded to fp32 on the host exactly where the
// literal expressions round (derived constants folded in double first: np_f16_host.h::make_airframe).  r_* = RN(1 / x) of a divisor
// (np_divc).  The defaults are the F-16 literals: a context built without an airframe block computes what the literals computed, bit for bit.
// A new field goes into three places: here, make_airframe and fleet_record (np_f16_host.h: the record of a fleet's table is copied field by
// field so that its padding is zero; a static_assert on the size stands there).
struct Airframe {
    float g, mass, r_mass, B, S, cbar, Heng, pad_;
    float Jy, r_Jy, Jxz, Jz, Jx;
    float xc, cbar_over_B, c1, c2, c3, c4, denom, r_denom;       // xcgr - xcg, cbar / B, the inertia products of the moment equations
    float ail_ref, r_ail_ref, rud_ref, r_rud_ref;                 // dail = ail / 21.5, drud = rud / 30
    float atm_lapse, rho0;                                        // tfac = 1 - 0.703e-5 alt; rho = 2.377e-3 tfac^4.14
    double atm_exp;                                               // (double)(float)4.14: the double np_pow computes in; > 0 (host check)
    float lag_keep, lag_new, thrust_frac, thrust_max, thrust_unit, r_thrust_unit, surf_max[3];   // u' = 0.9 u + 0.1 a * scale
    NP_DEVICE_INLINE const Airframe &get() const { return *this; }
};

// A fleet (np_f16_set_fleet / np_f16_set_fleet_index): K airframe records in device memory, each exactly what make_airframe gives for its
// class (np_f16_host.h::fleet_table; padding bytes zero), and the class of every row of the batch.  Row i flies table[index[i]].
struct FleetRef {
    const Airframe *table;   // [k], 16-byte aligned (records are whole 16-byte vectors: the kernels load them as such)
    const int *index;        // [rows of the launch]
    unsigned k, pad_;
};
constexpr int FLEET_MAX_CLASSES = 65536;

// Scenario constants, pre-rounded on the host exactly where the reference rounds them.
struct DevCfg {
    float dt, airspeed, noise_scale;
    float altitude_limit, acceleration_limit, max_velocity, min_velocity;
    float min_alpha, max_alpha, min_beta, max_beta;
    long long max_check_interval, min_check_interval;
    float init_T, alt_span, min_altitude, vt_span, min_vt;
    float max_heading_increment, max_pitch_increment, max_velocities_u_increment;
    float dist_span, min_distance;
    int aero_1d_tables;  // single-input nets through their piecewise-linear tables instead of the MLP bodies
    Airframe af;
};

// SingleCombat (np_f16_combat.h): one attitude PID and the scenario constants
struct PidDev {
    float Kp, Ki, Kd, Kff, Kimax, tau, rmax_pos, rmax_neg;
    int ki_on;  // `self.Ki != 0 and self.dt > 0` (pid.py:38)
};

struct CombatDevCfg {
    float dt;        // integrator step t1 - t0 (F16_model.py:66)
    float dt_pid;    // Controller(dt=...) (singlecombat_env.py:46)
    float airspeed;
    float altitude_limit, acceleration_limit, max_velocity, min_velocity;
    float min_alpha, max_alpha, min_beta, max_beta;
    float dist_limit_sq;
    long long max_steps;
    float init_T;
    float alt_span, min_altitude, vt_span, min_vt, yaw_span, min_heading, npos_span, min_npos, epos_span, min_epos;
    PidDev roll, pitch, yaw;
    float roll_ff, gravity, scale_min, scale_max;
    int inner_steps;
    int aero_1d_tables;
    Airframe af;   // np_f16_combat_cfg.airframe (defaults: the F-16 literals)
};

}  // namespace npf16
