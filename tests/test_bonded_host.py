"""The specific interactions without a GPU: the fp64 oracle (oracle/oracle.cpp: specific_forces, specific_pe, the specific virial) against the independent numpy
reference of tests/bonded_ref.py — energies from their definitions, forces and virial by finite differences in longdouble — on the systems the device tests use
(tests/test_gpu_bonded.py), and the yardsticks those tests' fp32 bars are made of.

Measured here, on the CPU (`python -m tests.test_bonded_host` prints both tables):

ORACLE_VS_REF — fp64 oracle against the longdouble reference (4th-order central differences, step 1e-5 nm and 1e-5 strain; 1e-7 nm for the near-collinear angles),
worst over a group's systems of (per-atom ‖Δf_i‖/S_i, |ΔE|/|E|, max|ΔW|/max|W|).  Regular geometry: forces at most 7.2e-12·S_i (bead_torsions; bonds 5.8e-15), energy at
most 1.1e-15, virial at most 1.1e-12 (hub_mixed).  The host test's bar is ten times the group's figure (not below ten units of float64 roundoff).

YARD32 — the oracle's own arithmetic in fp32 (correctly rounded host libm) against itself in fp64, same three ratios, worst over 20 seeds of every regular system
(the 60-bead chain and the degenerate configurations are single systems).  The device's fp32 bar is twice the group's figure: it uses another libm and another
fma contraction than the host compiler, so the two legitimately differ by a small factor."""
import math

import numpy as np
import pytest

from tests import bonded_ref as R
from tests import systems as S  # noqa: F401  (Case.oracle)

# worst (‖Δf_i‖/S_i, |ΔE|/|E|, max|ΔW|/max|W|) of case.oracle(np.float32) against case.oracle(np.float64): measure(), seeds 0–19 of bonded_ref.regular_groups and
# bonded_ref.degenerate_groups.  For torsion_planar the force scale is bonded_ref.full_scale_torsions (S_i vanishes there).  For the two planar-torsion groups and
# the two near-collinear groups the virial scale is Ref.virial_scale (the tensor all but vanishes), and the device tests take the force figure for the virial
# (‖ΔW‖ ≤ worst ‖Δf‖/S · Σ‖r‖‖f‖).
YARD32 = {
    "a_bonds": (3.05e-05, 2.50e-06, 8.08e-06),
    "a_angles": (4.73e-04, 3.13e-05, 1.57e-05),
    "a_torsions": (7.89e-03, 5.16e-05, 3.92e-06),
    "a_excl": (2.64e-06, 2.85e-05, 1.96e-06),
    "a_mixed": (3.64e-04, 7.46e-07, 9.71e-06),
    "hub_bonds": (5.15e-06, 1.32e-06, 1.13e-05),
    "hub_mixed": (3.58e-04, 6.21e-06, 1.39e-05),
    "resort": (4.62e-04, 3.44e-07, 9.36e-07),
    "tri": (2.07e-04, 8.34e-07, 4.20e-06),
    "bead_all": (6.91e-06, 1.21e-06, 1.86e-06),
    "bead_bonds": (1.32e-05, 6.64e-07, 2.21e-06),
    "bead_angles": (2.74e-05, 3.28e-07, 3.18e-06),
    "bead_torsions": (1.33e-05, 2.43e-07, 5.15e-06),
    "bead_excl": (2.90e-06, 4.07e-07, 6.72e-07),
    "near_collinear_1e-3": (2.59e-05, 2.64e-05, 6.79e-09),
    "near_collinear_1e-5": (7.23e-06, 1.26e-05, 3.20e-11),
    "torsion_planar": (6.76e-07, 8.29e-16, 0.00e+00),
    "torsion_near_pi": (2.47e-03, 5.46e-13, 2.96e-09),
    "excl_pairs": (7.68e-05, 1.87e-07, 2.72e-07),
    "face_bonds": (0.00e+00, 0.00e+00, 0.00e+00),
}
# the same three ratios of case.oracle(np.float64) against the longdouble reference: seed 0 of the regular groups, the degenerate groups as they are
ORACLE_VS_REF = {
    "a_bonds": (4.72e-15, 8.46e-16, 4.03e-13),
    "a_angles": (1.55e-13, 1.08e-15, 4.21e-13),
    "a_torsions": (4.02e-12, 3.57e-16, 9.03e-13),
    "a_excl": (4.48e-14, 2.38e-16, 6.64e-13),
    "a_mixed": (1.15e-13, 8.37e-16, 4.14e-13),
    "hub_bonds": (5.76e-15, 6.62e-16, 6.31e-13),
    "hub_mixed": (6.12e-14, 5.81e-16, 1.12e-12),
    "resort": (7.72e-15, 1.43e-16, 6.26e-13),
    "tri": (3.94e-13, 8.69e-16, 2.07e-13),
    "bead_all": (6.62e-13, 0.00e+00, 8.97e-14),
    "bead_bonds": (3.61e-15, 2.40e-16, 8.51e-14),
    "bead_angles": (7.39e-13, 3.62e-16, 2.28e-13),
    "bead_torsions": (7.22e-12, 3.88e-16, 7.01e-13),
    "bead_excl": (3.23e-14, 2.45e-16, 1.84e-13),
    "near_collinear_1e-3": (3.18e-13, 4.38e-14, 2.35e-13),
    "near_collinear_1e-5": (8.39e-12, 1.10e-11, 1.60e-13),
    "torsion_planar": (7.53e-16, 1.18e-16, 0.00e+00),
    "torsion_near_pi": (2.25e-11, 0.00e+00, 6.61e-13),
    "excl_pairs": (2.76e-13, 0.00e+00, 5.82e-14),
    "face_bonds": (2.52e-15, 0.00e+00, 1.02e-12),
}
# worst per-atom ‖Δv_i‖/V_i (bonded_ref.velocity_scale) after RUN_STEPS velocity-Verlet steps from rest of bonded_ref.fluid_with_chains, fp32 oracle run against
# fp64 oracle run, seeds 0–19
RUN_STEPS = 2
YARD32_RUN = {"rf": 7.04e-05, "pme": 8.53e-05}

EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23      # a figure below one unit of roundoff only says the host's arithmetic happened to be exact on those inputs: bars stop there


def measure(seeds=range(20)):
    y32, y64 = {}, {}
    upd = lambda d, k, v: d.__setitem__(k, tuple(max(a, b) for a, b in zip(d.get(k, (0.0, 0.0, 0.0)), v)))
    for seed in seeds:
        for g, cases in R.regular_groups(seed).items():
            for c in cases:
                sc = R.group_scale(g, c)
                upd(y32, g, R.fp32_yardstick(c, scale=sc))
                if seed == 0:
                    upd(y64, g, R.oracle_vs_ref(g, c, sc))
    for g, cases in R.degenerate_groups().items():
        for c in cases:
            sc = R.group_scale(g, c)
            upd(y32, g, R.fp32_yardstick(c, scale=sc, wscale=R.group_wscale(g, c))); upd(y64, g, R.oracle_vs_ref(g, c, sc))
    return y32, y64


def measure_run(seeds=range(20)):
    out = {}
    for kind in ("rf", "pme"):
        for seed in seeds:
            c = R.fluid_with_chains(kind, seed)
            r = np.linalg.norm(R.oracle_run(c, np.float32, RUN_STEPS) - R.oracle_run(c, np.float64, RUN_STEPS), axis=1) / R.velocity_scale(c, RUN_STEPS)
            out[kind] = max(out.get(kind, 0.0), float(r.max()))
    return out


_GROUPS0 = None


def groups0():
    global _GROUPS0
    if _GROUPS0 is None:
        _GROUPS0 = {**R.regular_groups(0), **R.degenerate_groups()}
    return _GROUPS0


@pytest.mark.parametrize("group", sorted(ORACLE_VS_REF))
def test_oracle_specific_terms_agree_with_the_independent_reference(group):
    """Forces, energy and virial of the fp64 oracle against energies-from-definitions differentiated numerically in longdouble: every type alone at 1, 63, 64, 65 and
    129 terms, all types together, cubic and triclinic, the hub systems, the 60-bead chain, the near-degenerate configurations.  Measured (ORACLE_VS_REF): forces
    within 7.2e-12·S_i per atom on regular geometry (bead_torsions; 8.4e-12·S_i for the angles 1e-5 rad off collinear), energy within 1.1e-15 (1.1e-11 near collinear: acos),
    virial within 1.1e-12 of its largest component.  Bar: ten times the group's figure.  The oracle's tensor is
    symmetric to rounding.  Every atom with S_i > 0 is compared; nothing here is exactly collinear or coincident."""
    for case in groups0()[group]:
        assert not R.nondifferentiable_terms(case)
        scale = R.group_scale(group, case)
        slots = R.slot_counts(case)
        assert not np.any((scale > 0) & (slots == 0))
        if group != "torsion_planar":
            assert np.array_equal(scale > 0, (slots > 0) & ~zero_charge_only(case, slots))
        f, e, w = R.oracle_all(case, np.float64)
        assert np.abs(w - w.T).max() <= 1e-12 * (R.group_wscale(group, case) or np.abs(w).max())
        rf, re, rw = R.oracle_vs_ref(group, case, scale)
        bf, be, bw = (10.0 * max(v, EPS64) for v in ORACLE_VS_REF[group])
        assert rf <= bf and re <= be and rw <= bw, (case.name, (rf, re, rw), (bf, be, bw))


def zero_charge_only(case, slots):
    """atoms whose only terms are exclusions with a zero product of charges: no force by definition"""
    if case.ewald_excl is None or case.bonds is not None or case.angles is not None or case.torsions is not None:
        return np.zeros(case.n, bool)
    e = np.asarray(case.ewald_excl).reshape(-1, 2)
    live = np.zeros(case.n, bool)
    qq = case.charge[e[:, 0]] * case.charge[e[:, 1]]
    live[e[qq != 0].reshape(-1)] = True
    return (slots > 0) & ~live


def test_degenerate_geometry_gives_what_the_definitions_say():
    """Exactly collinear angles (straight and folded): no force, energy k/2 (θ − θ0)² with θ = π and 0.  Coincident charges: no force, energy −2α·ke·qi·qj/√π per
    pair.  A bond at r = r0: nothing.  These are the only configurations the finite-difference reference is not asked about (the energy has no derivative there)."""
    flat = R.collinear_angles()
    assert {k: list(v) for k, v in R.nondifferentiable_terms(flat).items()} == {"angles": [0, 1]}
    f, e, w = R.oracle_all(flat, np.float64)
    e_def = 384.0 / 2 * (math.pi - 1.75) ** 2 + 384.0 / 2 * 1.75 ** 2
    assert np.all(f == 0.0) and np.all(w == 0.0) and e == pytest.approx(e_def, rel=1e-15) and float(R.energy(flat)) == pytest.approx(e_def, rel=1e-15)
    assert not R.nondifferentiable_terms(R.collinear_angles(bent=True))
    co = R.exclusion_pairs(coincident=True)
    assert {k: list(v) for k, v in R.nondifferentiable_terms(co).items()} == {"excl": [0, 1]}
    f, e, w = R.oracle_all(co, np.float64)
    alpha = co.inter_dict(np.float64)["ewald_alpha"]
    e_def = 2 * (-2.0 * alpha * R.KE * (0.5 * -0.75) / math.sqrt(math.pi))
    assert np.all(f == 0.0) and e == pytest.approx(e_def, rel=1e-15) and float(R.energy(co)) == pytest.approx(e_def, rel=1e-15)
    for dtype in (np.float64, np.float32):
        f, e, w = R.oracle_all(R.exact_bond(), dtype)
        assert np.all(f == 0.0) and e == 0.0 and np.all(w == 0.0)
    # the reference's two erf forms agree: the series used everywhere against the limit and against math.erf
    r = R.of_case(co)
    for x in (0.0, 1e-9, 0.3, 2.6):
        got = float(R._erf_over_x(np.array([x], dtype=np.longdouble), np.longdouble)[0])
        assert got == pytest.approx(2.0 / math.sqrt(math.pi) if x == 0.0 else math.erf(x) / x, rel=4e-16)


def test_fp32_yardsticks_are_what_the_oracle_measures():
    """YARD32 (the module docstring says how it was measured): the first seed of every group and the single systems again — nothing measured exceeds the recorded
    figure, and the single systems' figures are the recorded ones.  Forces: bonds 3.1e-5·S_i, angles 4.7e-4, torsions 7.9e-3 (a torsion whose sin(nφ − phase) is
    small loses that much to the rounding of φ), exclusions 2.6e-6, mixed systems 3.6e-4; energy at most 5.2e-5, virial at most 1.6e-5 of the largest component."""
    single = set(R.degenerate_groups()) | {g for g in YARD32 if g.startswith("bead_")}
    for g, cases in groups0().items():
        worst = (0.0, 0.0, 0.0)
        for c in cases:
            worst = tuple(max(a, b) for a, b in zip(worst, R.fp32_yardstick(c, scale=R.group_scale(g, c), wscale=R.group_wscale(g, c))))
        for got, rec in zip(worst, YARD32[g]):
            assert got <= 1.01 * rec + 1e-300, (g, worst, YARD32[g])
            if g in single:
                assert got >= 0.99 * rec, (g, worst, YARD32[g])


def test_run_yardstick_and_the_shape_of_the_fluid_with_chains():
    for kind in ("rf", "pme"):
        c = R.fluid_with_chains(kind)
        nt = R.n_terms(c)
        assert (nt["bonds"], nt["angles"], nt["torsions"], nt["excl"]) == (70, 65, 130, 0) and abs(c.charge.sum()) < 1e-5
        r = np.linalg.norm(R.oracle_run(c, np.float32, RUN_STEPS) - R.oracle_run(c, np.float64, RUN_STEPS), axis=1) / R.velocity_scale(c, RUN_STEPS)
        assert r.max() <= 1.01 * YARD32_RUN[kind]


if __name__ == "__main__":
    fmt = lambda d: "{\n" + "".join(f'    "{k}": ({v[0]:.2e}, {v[1]:.2e}, {v[2]:.2e}),\n' for k, v in d.items()) + "}"
    a, b = measure()
    print("YARD32 =", fmt(a)); print("ORACLE_VS_REF =", fmt(b)); print("YARD32_RUN =", measure_run())
