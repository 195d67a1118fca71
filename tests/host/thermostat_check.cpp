// thermostat_check.cpp — the rescaling thermostats' λ (molly.jl_amd/csrc/thermostat.h) on the host, alone: known answers against closed forms,
// the identities between the kinds, the guards, and the centre-of-mass identity of K against an explicit sum on seeded inputs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "thermostat.h"

using namespace mhip;

static int n_fail = 0;
static void check(bool ok, const char* what, double got = 0, double want = 0) {
    if (!ok) { ++n_fail; std::printf("FAIL %s: got %.17g, want %.17g\n", what, got, want); }
}
static bool close_rel(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

// a small generator of its own (splitmix64): the inputs are seeded, not the library's noise
static uint64_t sm_state = 0x9E3779B97F4A7C15ull;
static double uni() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

int main() {
    const double kT = 2.494338785445972;      // k · 300 K
    const double P0[3] = {0, 0, 0};
    const int64_t dof = 597;
    const double Kbar = 0.5 * (double)dof * kT;

    // ---- known answers ------------------------------------------------------------------------------------------------------------
    {   // Immediate: K = Kbar / 4 → λ = 2; K = 4·Kbar → λ = 1/2
        double K = 0; int32_t ref = -1;
        double l = thermostat_lambda(THERMO_IMMEDIATE, 2 * (Kbar / 4), P0, 1.0, false, dof, kT, 0.002, 1.0, 1, 0, 0, &K, &ref);
        check(close_rel(l, 2.0, 1e-15), "immediate, K = Kbar/4", l, 2.0);
        check(close_rel(K, Kbar / 4, 1e-15) && ref == 0, "immediate: K reported, not refused", K, Kbar / 4);
        l = thermostat_lambda(THERMO_IMMEDIATE, 2 * (4 * Kbar), P0, 1.0, false, dof, kT, 0.002, 1.0, 1, 0, 0);
        check(close_rel(l, 0.5, 1e-15), "immediate, K = 4 Kbar", l, 0.5);
    }
    {   // Berendsen: dt/τ = 0.1, Kbar/K = 2 → λ² = 1.1; Kbar/K = 0.5 → λ² = 0.95
        double l = thermostat_lambda(THERMO_BERENDSEN, 2 * (Kbar / 2), P0, 1.0, false, dof, kT, 0.002, 0.02, 1, 0, 0);
        check(close_rel(l, std::sqrt(1.1), 1e-15), "berendsen, Kbar/K = 2", l, std::sqrt(1.1));
        l = thermostat_lambda(THERMO_BERENDSEN, 2 * (2 * Kbar), P0, 1.0, false, dof, kT, 0.002, 0.02, 1, 0, 0);
        check(close_rel(l, std::sqrt(0.95), 1e-15), "berendsen, Kbar/K = 1/2", l, std::sqrt(0.95));
    }
    {   // CSVR: c = exp(−1) (dt·n_steps = τ), K = Kbar, R = 0.5, S = dof − 1: A = 1/dof
        const double c = std::exp(-1.0), A = 1.0 / (double)dof, R = 0.5, S = (double)(dof - 1);
        const double want = std::sqrt(c + (1 - c) * A * (R * R + S) + 2 * std::sqrt(c * (1 - c) * A) * R);
        double l = thermostat_lambda(THERMO_CSVR, 2 * Kbar, P0, 1.0, false, dof, kT, 0.002, 0.008, 4, R, S);
        check(close_rel(l, want, 1e-15), "csvr closed form, n_steps = 4", l, want);
        // n_steps enters only through dt·n_steps
        double l2 = thermostat_lambda(THERMO_CSVR, 2 * Kbar, P0, 1.0, false, dof, kT, 0.008, 0.008, 1, R, S);
        check(l == l2, "csvr: dt·n_steps", l2, l);
    }
    // ---- identities ---------------------------------------------------------------------------------------------------------------
    for (int k = 0; k < 1000; ++k) {
        const double K = Kbar * (0.05 + 4 * uni()), dt = 0.0005 + 0.004 * uni();
        const double li = thermostat_lambda(THERMO_IMMEDIATE, 2 * K, P0, 1.0, false, dof, kT, dt, 7.0, 1, 0, 0);
        const double lb = thermostat_lambda(THERMO_BERENDSEN, 2 * K, P0, 1.0, false, dof, kT, dt, dt, 1, 0, 0);
        check(close_rel(li, lb, 4e-16), "berendsen with tau = dt equals immediate", lb, li);
        // c → 0: K λ² = ½ kT (R² + S)
        const double R = 4 * uni() - 2, S = (double)dof * (0.5 + uni());
        const double l0 = thermostat_lambda(THERMO_CSVR, 2 * K, P0, 1.0, false, dof, kT, dt, 1e-9, 1, R, S);
        check(close_rel(K * l0 * l0, 0.5 * kT * (R * R + S), 1e-14), "csvr with c -> 0: K lambda^2 = kT/2 (R^2 + S)", K * l0 * l0, 0.5 * kT * (R * R + S));
        // τ → ∞: λ = 1
        const double l1 = thermostat_lambda(THERMO_CSVR, 2 * K, P0, 1.0, false, dof, kT, dt, 1e300, 1, R, S);
        check(l1 == 1.0, "csvr with tau -> inf: lambda = 1", l1, 1.0);
    }
    // ---- guards -------------------------------------------------------------------------------------------------------------------
    for (int kind = THERMO_IMMEDIATE; kind <= THERMO_CSVR; ++kind) {
        int32_t ref = 0;
        double l = thermostat_lambda(kind, 2 * Kbar, P0, 1.0, false, 0, kT, 0.002, 0.1, 1, 0.3, 100.0, nullptr, &ref);
        check(l == 1.0 && ref == 1, "dof = 0: lambda = 1, refused", l, 1.0);
        l = thermostat_lambda(kind, 0.0, P0, 1.0, false, dof, kT, 0.002, 0.1, 1, 0.3, 100.0, nullptr, &ref);
        check(l == 1.0 && ref == 1, "K = 0: lambda = 1, refused", l, 1.0);
        const double Pm[3] = {3, 4, 0};      // K = ½·25 − ½·25/1 = 0 once the centre-of-mass motion is removed
        l = thermostat_lambda(kind, 25.0, Pm, 1.0, true, dof, kT, 0.002, 0.1, 1, 0.3, 100.0, nullptr, &ref);
        check(l == 1.0 && ref == 1, "K = 0 behind the CM removal: lambda = 1, refused", l, 1.0);
    }
    {   // Berendsen with dt/τ = 3, K = 4·Kbar: λ² = 1 + 3·(¼ − 1) < 0 → λ = 1, refused
        int32_t ref = 0;
        double l = thermostat_lambda(THERMO_BERENDSEN, 2 * (4 * Kbar), P0, 1.0, false, dof, kT, 0.003, 0.001, 1, 0, 0, nullptr, &ref);
        check(l == 1.0 && ref == 1, "berendsen, negative lambda^2: lambda = 1, refused", l, 1.0);
    }
    {   // CSVR: R strongly negative drives λ² below zero only through rounding; the floor is DBL_EPSILON.  c(1−c)A R² + … : pick S = 0, R = −sqrt(c/((1−c)A)) → λ² = (sqrt(c) − sqrt((1−c) A) |R|)² = 0
        const double c = std::exp(-0.5), A = 1.0 / (double)dof;
        const double R = -std::sqrt(c / ((1 - c) * A));
        int32_t ref = -1;
        double l = thermostat_lambda(THERMO_CSVR, 2 * Kbar, P0, 1.0, false, dof, kT, 0.002, 0.004, 1, R, 0.0, nullptr, &ref);
        check(l >= std::sqrt(2.220446049250313e-16) && l < 1e-6 && ref == 0, "csvr floor at DBL_EPSILON", l, std::sqrt(2.220446049250313e-16));
    }
    {   // kind 0 and out-of-range kinds leave the velocities alone
        check(thermostat_lambda(0, 2 * Kbar, P0, 1.0, false, dof, kT, 0.002, 0.1, 1, 0, 0) == 1.0, "kind 0");
        check(thermostat_lambda(7, 2 * Kbar, P0, 1.0, false, dof, kT, 0.002, 0.1, 1, 0, 0) == 1.0, "kind 7");
    }
    // ---- the centre-of-mass identity: ½ Σ m|v|² − ½ |P|²/M = Σ ½ m |v − v_cm|² ---------------------------------------------------
    int n_sweep = 0;
    for (int trial = 0; trial < 200; ++trial) {
        const int n = 2 + (int)(uni() * 500);
        std::vector<double> m(n), v(3 * n);
        double P[3] = {0, 0, 0}, M = 0, s2 = 0;
        const double drift[3] = {4 * uni() - 2, 4 * uni() - 2, 4 * uni() - 2};
        for (int i = 0; i < n; ++i) {
            m[i] = 1.0 + 15.0 * uni();
            for (int d = 0; d < 3; ++d) { v[3 * i + d] = drift[d] + (2 * uni() - 1); P[d] += m[i] * v[3 * i + d]; s2 += m[i] * v[3 * i + d] * v[3 * i + d]; }
            M += m[i];
        }
        double K_explicit = 0;
        for (int i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) { const double w = v[3 * i + d] - P[d] / M; K_explicit += 0.5 * m[i] * w * w; }
        const double K = thermostat_kinetic(s2, P, M, true);
        check(close_rel(K, K_explicit, 1e-12), "CM identity", K, K_explicit);
        check(thermostat_kinetic(s2, P, M, false) == 0.5 * s2, "no CM removal: K = sum/2");
        ++n_sweep;
    }
    std::printf("sweep: %d seeded velocity sets\n", n_sweep);
    if (n_fail) { std::printf("%d checks failed\n", n_fail); return 1; }
    std::printf("all thermostat checks passed\n");
    return 0;
}
