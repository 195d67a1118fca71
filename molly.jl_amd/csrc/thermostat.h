// thermostat.h — the velocity scale λ of the rescaling thermostats (coupling.jl:68-238) from the sums the step loop takes on the device.
// One host+device function in double on a handful of scalars: no device code of its own, nothing of the engine
// (tests/host/thermostat_check.cpp runs it alone; the kernels of thermostat_step.h call it once per workgroup).
//
//   kind 1  ImmediateThermostat        λ  = sqrt(½·dof·kT / K)                                        coupling.jl:86-91, T = 2K/(dof·k)
//   kind 2  BerendsenThermostat        λ² = 1 + (dt/τ)·(½·dof·kT / K − 1)                             :232-238
//   kind 3  VelocityRescaleThermostat  λ² = c + (1 − c)·A·(R² + S) + 2·sqrt(c·(1 − c)·A)·R            :140-159
//           c = exp(−dt·n_steps/τ), A = (½·dof·kT)/(dof·K), R ~ N(0, 1), S ~ χ²(dof − 1); λ² floored at DBL_EPSILON
//
// K = ½·Σ m|v|², less ½·|P|²/M when the step removes centre-of-mass motion: the kinetic energy of v − v_cm exactly (the reference
// removes first and measures afterwards, simulators.jl:627-643).
// Deviations, both stated: dof <= 0 or K <= 0 gives λ = 1 for every kind (the reference returns early for kind 3 and divides by zero
// for the other two); a negative λ² of kinds 1, 2 — the reference's sqrt domain error — gives λ = 1 and *refused = 1.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MHIP_THERMO_HD __host__ __device__
#else
#define MHIP_THERMO_HD
#endif

namespace mhip {

enum : int32_t { THERMO_OFF = 0, THERMO_IMMEDIATE = 1, THERMO_BERENDSEN = 2, THERMO_CSVR = 3 };

// the kinetic energy the thermostat measures [kJ/mol]
MHIP_THERMO_HD inline double thermostat_kinetic(double sum_mv2, const double* P, double M, bool cm_removed) {
    double K = 0.5 * sum_mv2;
    if (cm_removed && M > 0) K -= 0.5 * (P[0] * P[0] + P[1] * P[1] + P[2] * P[2]) / M;
    return K;
}

// k_out (nullable): K as measured; refused (nullable): set to 1 when the application was refused (K <= 0, dof <= 0, negative λ²), else 0
MHIP_THERMO_HD inline double thermostat_lambda(int32_t kind, double sum_mv2, const double* P, double M, bool cm_removed, int64_t dof, double kT, double dt,
                                               double tau, int32_t n_steps, double R, double S, double* k_out = nullptr, int32_t* refused = nullptr) {
    const double K = thermostat_kinetic(sum_mv2, P, M, cm_removed);
    if (k_out) *k_out = K;
    if (refused) *refused = 0;
    if (kind < THERMO_IMMEDIATE || kind > THERMO_CSVR) return 1.0;
    if (dof <= 0 || !(K > 0)) { if (refused) *refused = 1; return 1.0; }
    const double Kbar = 0.5 * (double)dof * kT;
    double lam2;
    if (kind == THERMO_IMMEDIATE) lam2 = Kbar / K;
    else if (kind == THERMO_BERENDSEN) lam2 = 1.0 + (dt / tau) * (Kbar / K - 1.0);
    else {
        const double c = std::exp(-(dt * (double)n_steps) / tau);
        const double A = Kbar / ((double)dof * K);
        lam2 = c + (1.0 - c) * A * (R * R + S) + 2.0 * std::sqrt(c * (1.0 - c) * A) * R;
        const double eps = 2.220446049250313e-16;      // DBL_EPSILON (eps(Float64), :158)
        if (!(lam2 > eps)) lam2 = eps;
        return std::sqrt(lam2);
    }
    if (!(lam2 >= 0)) { if (refused) *refused = 1; return 1.0; }
    return std::sqrt(lam2);
}

// what the launches of a coupled step are handed (thermostat_step.h)
struct ThermoP {
    int32_t kind = 0, n_steps = 1;
    int64_t dof = 0, step = 0;           // step: the step this application closes (the info record's)
    double kT = 0, dt = 0, tau = 1;
    uint64_t key = 0, ctr1 = 0, natoms = 0;      // ctr1: the caller's + step
    double* info = nullptr;              // the 8 doubles of mhip_thermostat_info, updated by the first lane of block 0
};

// … and the partial arrays of a coupled step: the close launch writes th_out, the open launch and the flush read th_in
struct ThermoArgs {
    ThermoP th;
    const double* th_in = nullptr;
    double* th_out = nullptr;
};

}  // namespace mhip
