"""Reciprocal-space PME without a GPU: the fp64 oracle (oracle/pme.h — the same algorithm as the engine's, restated) against the exact Ewald sum over wave vectors
of tests/pme_ref.py, which shares nothing with either; the index arithmetic of the spreading paths on hand-made batches; and the yardsticks the fp32 run bars of
tests/test_gpu_pme_edges.py are made of.

Measured here, on the CPU (`python -m tests.test_pme_host` prints the tables):

ORACLE_VS_EWALD — 24 random charges, order 6, cell (2.0, 2.3, 2.6) nm, mesh (64, 72, 80), wave vectors |m_d| ≤ 14: (worst ‖Δf_i‖ / largest ‖f_i‖, |ΔE|/|E|,
max|ΔW|/max|W|) of the oracle against the exact sum — orthorhombic, sheared, and with a net charge of +3 e.  What is left is the discretisation error of a
sixth-order PME on a mesh of 0.03 nm.  CONVERGENCE — the same orthorhombic system on mesh (32, 36, 40) with orders 4, 5 and 6.  The bars are ten times the figures.

YARD32_RUN — worst per-atom ‖Δv_i‖/V_i (bonded_ref.velocity_scale) after RUN_STEPS velocity-Verlet steps from rest of charged_with_chains (every atom charged,
bonded terms present), the oracle's fp32 run against its fp64 run, worst over seeds 0–19, per B-spline order.  The device's fp32 bar is twice the figure (another
libm, another fma contraction than the host compiler's)."""
import numpy as np
import pytest

from tests import bonded_ref as B
from tests import pme_ref as R
from tests import systems as S  # noqa: F401  (Case.oracle)
from tests.test_bonded_host import RUN_STEPS

CELL, FINE, COARSE = (2.0, 2.3, 2.6), (64, 72, 80), (32, 36, 40)
SHEARED = [[2.0, 0.0, 0.0], [0.5, 2.3, 0.0], [0.3, -0.4, 2.6]]
LARGE_SIDE = 33            # 35 937 fluid atoms + the chains: beyond the group-split launch, and the second batch round of the integrating launch
CLEAR = 0.15               # nm: fluid atoms closer than this to a chain atom are left out of charged_with_chains

ORACLE_VS_EWALD = {
    "orthorhombic": (8.96e-08, 4.01e-09, 1.72e-08),
    "sheared": (1.05e-07, 4.26e-09, 1.85e-08),
    "net_charge": (1.04e-07, 3.81e-09, 1.95e-08),
}
CONVERGENCE = {
    4: (4.45e-04, 3.78e-05, 1.17e-04),
    5: (1.78e-05, 1.29e-06, 6.45e-06),
    6: (3.37e-06, 2.56e-07, 1.27e-06),
}
YARD32_RUN = {
    "small_o4": 2.57e-05,
    "small_o5": 2.56e-05,
    "small_o6": 2.55e-05,
    "large_o5": 1.29e-04,
}


def ewald_case(which, order=6, mesh=FINE):
    if which == "sheared":
        return R.random_charges(24, None, order, mesh, dtype=np.float64, basis=SHEARED)
    return R.random_charges(24, CELL, order, mesh, dtype=np.float64, net=3.0 if which == "net_charge" else 0.0, name=which)


_exact = {}


def exact(which):
    """the exact sum of a system: once, shared, never modified"""
    if which not in _exact:
        c = ewald_case(which)
        e, f, w = R.ewald_reciprocal(c.coords, c.charge, R.basis_of(c), R.alpha_of(c))
        f.setflags(write=False); w.setflags(write=False)
        _exact[which] = (f, e, w)
    return _exact[which]


def oracle_vs_ewald(which, order=6, mesh=FINE):
    f_ref, e_ref, w_ref = exact(which)
    f, e, w = R.oracle_pme(ewald_case(which, order, mesh))
    return R.ratios(f, e, w, f_ref, e_ref, w_ref)


def charged_with_chains(order=5, seed=0, n_side=12, dtype=np.float32):
    """S.charged_fluid(n_side, stable=True) with the chains of bonded_ref.chains (70 bonds, 65 angles, 130 torsion entries) added as further atoms: every atom carries
    a charge, bonded terms are present, at rest.  The chain atoms have no core, so the fluid atoms within CLEAR of one are taken out (the fluid is the same for
    every seed, the chains are not).  The chains' 1-2 and 1-3 pairs are excluded from the pair list."""
    fl = S.charged_fluid(n_side, dict(kind="ewald", rc=1.0), dtype=dtype, with_exceptions=False, stable=True)
    ch = B.chains(n_bonds=70, n_angles=65, n_torsions=130, seed=seed, box=float(fl.box[0]), dtype=dtype)
    d = fl.coords[:, None, :] - ch.coords[None, :, :]; d -= np.round(d / fl.box) * fl.box
    keep = np.linalg.norm(d, axis=2).min(axis=1) >= CLEAR      # (a fluid charge on top of a chain atom without a core: forces of 1e5 that move it by half its distance per step)
    for k in ("coords", "charge", "sigma", "eps", "mass"):
        setattr(fl, k, getattr(fl, k)[keep])
    fl.n = int(keep.sum())
    n0, n1 = fl.n, ch.n
    off = lambda d, keys: {k: (np.asarray(v) + n0 if k in keys else np.asarray(v)) for k, v in d.items()}
    excl = np.concatenate([np.stack([c[:-1], c[1:]], 1) for c in ch.topo_chains] + [np.stack([c[:-2], c[2:]], 1) for c in ch.topo_chains]) + n0
    q = np.concatenate([fl.charge - fl.charge.mean(), ch.charge - ch.charge.mean()]).astype(dtype).astype(np.float64)
    case = S.Case(np.concatenate([fl.coords, ch.coords]), fl.box, lj=dict(cutoff=("distance", 1.0)), coul=dict(kind="ewald", rc=1.0), r_list=1.2, rebuild_every=10,
                  velocities=np.zeros((n0 + n1, 3)), charge=q, sigma=np.concatenate([fl.sigma, np.full(n1, 0.2)]), eps=np.concatenate([fl.eps, np.zeros(n1)]),
                  mass=np.concatenate([fl.mass, np.full(n1, 12.0)]), excluded=excl, bonds=off(ch.bonds, "ij"), angles=off(ch.angles, "ijk"),
                  torsions=off(ch.torsions, "ijkl"), pme=dict(order=order), name=f"charged_chains_{n_side}_o{order}_s{seed}")
    case.n_fluid = n0
    return case


def run_ratio(case, dtype, ref=None):
    ref = B.oracle_run(case, np.float64, RUN_STEPS) if ref is None else ref
    return np.linalg.norm(B.oracle_run(case, dtype, RUN_STEPS) - ref, axis=1) / B.velocity_scale(case, RUN_STEPS)


def measure_run(seeds=range(20)):
    out = {}
    for order in (4, 5, 6):
        out[f"small_o{order}"] = max(float(run_ratio(charged_with_chains(order, seed), np.float32).max()) for seed in seeds)
    out["large_o5"] = max(float(run_ratio(charged_with_chains(5, seed, n_side=LARGE_SIDE), np.float32).max()) for seed in seeds)
    return out


# ---- the oracle against the exact sum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["orthorhombic", "sheared", "net_charge"])
def test_oracle_reciprocal_space_agrees_with_the_exact_ewald_sum(which):
    """energy (self and net-charge terms included), forces per atom and the virial tensor of the fp64 oracle, order 6 on a 0.03 nm mesh, against the sum over wave
    vectors: bars ten times ORACLE_VS_EWALD.  All 24 atoms are compared; the reference's own virial is symmetric to the accuracy of its differences."""
    f_ref, e_ref, w_ref = exact(which)
    assert f_ref.shape == (24, 3) and np.all(np.linalg.norm(f_ref, axis=1) > 0) and np.abs(w_ref - w_ref.T).max() < 1e-9 * np.abs(w_ref).max()
    if which == "net_charge":
        assert ewald_case(which).charge.sum() == pytest.approx(3.0, abs=1e-12)
    got = oracle_vs_ewald(which)
    print(f"[pme host] {which}: forces {got[0]:.2e}, energy {got[1]:.2e}, virial {got[2]:.2e}")
    for g, rec in zip(got, ORACLE_VS_EWALD[which]):
        assert g <= 10.0 * rec, (which, got, ORACLE_VS_EWALD[which])


def test_the_net_charge_term_is_what_separates_the_charged_system():
    """the reference's three parts separately: a uniform shift of all charges by δ changes Σq, so the net-charge term −ke·π(Σq)²/(2Vα²) must be in the oracle's energy
    and on the diagonal of its virial — without it the two would disagree by far more than the bar"""
    c = ewald_case("net_charge")
    term = R.KE * np.pi * c.charge.sum() ** 2 / (2 * np.prod(c.box) * R.alpha_of(c) ** 2)
    f_ref, e_ref, w_ref = exact("net_charge")
    assert term > 1e3 * 10 * ORACLE_VS_EWALD["net_charge"][1] * abs(e_ref) and term > 1e3 * 10 * ORACLE_VS_EWALD["net_charge"][2] * np.abs(w_ref).max()


def test_orders_4_5_6_converge_on_a_coarser_mesh():
    """mesh (32, 36, 40): every order within ten times its recorded figure, and each order better than the one below it"""
    got = {o: oracle_vs_ewald("orthorhombic", o, COARSE) for o in (4, 5, 6)}
    print("[pme host] convergence:", {o: tuple(f"{v:.2e}" for v in g) for o, g in got.items()})
    for o, g in got.items():
        for v, rec in zip(g, CONVERGENCE[o]):
            assert v <= 10.0 * rec, (o, g, CONVERGENCE[o])
    assert got[4][0] > got[5][0] > got[6][0] and got[4][1] > got[5][1] > got[6][1]


def test_exact_sum_forces_are_the_gradient_of_its_energy():
    """the reference against itself: analytic forces against central differences of its energy in longdouble, and the cut-off of the sum (|m| ≤ 14 against 17)"""
    c = ewald_case("sheared")
    x, q, bv, al = c.coords, c.charge, R.basis_of(c), R.alpha_of(c)
    f_ref, e_ref, _ = exact("sheared")
    h = np.longdouble(1e-4)
    for i, d in ((0, 0), (7, 1), (23, 2)):
        def at(k):
            y = np.asarray(x, dtype=np.longdouble).copy(); y[i, d] += k * h
            return R._energy_forces(y, q, bv, al, R.KE, 14, np.longdouble, False)[0]
        g = -float((at(-2) - 8 * at(-1) + 8 * at(1) - at(2)) / (12 * h))
        assert abs(g - f_ref[i, d]) < 1e-9 * np.linalg.norm(f_ref, axis=1).max()
    e10, f10 = R._energy_forces(x, q, bv, al, R.KE, 17, np.float64, True)
    assert abs(float(e10) - e_ref) < 1e-13 * abs(e_ref) and np.abs(f10 - f_ref).max() < 1e-12 * np.abs(f_ref).max()


# ---- the spreading paths ---------------------------------------------------------------------------------------------
def test_spread_paths_on_hand_made_batches():
    """mesh 32³, box 2.4 nm (spacing 0.075 nm), order 4, batches of 64"""
    box, mesh, sp = 2.4, (32, 32, 32), 0.075
    T = np.float32
    rng = np.random.default_rng(1)
    near = lambda c, m: (np.asarray(c) + rng.uniform(0, 3 * sp, (m, 3))).astype(T)
    x = np.concatenate([near([1.0, 1.0, 1.0], 64),                      # a cluster of 3 spacings: extents 4 + 3 = 7 per axis, 343 cells
                        rng.uniform(0, box, (64, 3)).astype(T),          # all over the box: extents beyond the mesh
                        near([0.3, 0.3, 0.3], 64),                      # the same cluster, every charge zero
                        (near([-1.5 * sp] * 3, 64) % T(box)).astype(T),  # the cluster across the corner: folded, it is as compact as the first
                        near([2.0, 0.5, 1.0], 64), near([0.5, 2.0, 1.0], 10)])
    q = np.ones(len(x)); q[128:192] = 0.0
    q[256] = 24.0; q[320] = np.nextafter(np.float32(24.0), np.float32(np.inf))
    assert R.spread_paths(x, q, mesh, 4, (box,) * 3) == ["lds", "direct", "empty", "lds", "lds", "direct"]
    q[320] = 1.0; q[321:] = 0.0                                          # a single charge in a short last batch
    assert R.spread_paths(x, q, mesh, 4, (box,) * 3)[-1] == "lds"
    # the zero charges of a batch do not count into its box: one charged atom among atoms all over the box still fits
    q[64:128] = 0.0; q[100] = -0.5
    assert R.spread_paths(x, q, mesh, 4, (box,) * 3)[1] == "lds"
    # 6144 cells: extents (order + span) of 18 · 18 · 19 = 6156 do not fit, 18 · 18 · 18 do (mesh 96³, order 6)
    for span_z, want in ((12, "lds"), (13, "direct")):
        y = np.zeros((2, 3), np.float64); y[1] = np.array([12, 12, span_z]) * (box / 96)
        assert R.spread_paths((y + 0.5 * box / 96).astype(np.float64), np.ones(2), (96,) * 3, 6, (box,) * 3) == [want]


def test_placement_on_nodes_and_at_the_top_of_the_box():
    """an atom on mesh node k has first index k and offset 0 (box 2.0 nm: 1/L, the spacing and the nodes are exact in both precisions); the largest float below L lands in the last cell, not on n"""
    for T in (np.float32, np.float64):
        box = T(2.0); n = 32                                             # spacing 1/16 nm
        x = np.array([[0.0, 0.0625 * 7, np.nextafter(box, T(0))]], dtype=T)
        idx, dr = R.place(x, (n,) * 3, (float(box),) * 3)
        assert idx.tolist() == [[0, 7, n - 1]] and dr[0, 0] == 0 and dr[0, 1] == 0 and 0.99 < dr[0, 2] < 1


# ---- the run yardsticks ----------------------------------------------------------------------------------------------
def test_run_yardstick_and_the_shape_of_the_charged_system():
    for order in (4, 5, 6):
        c = charged_with_chains(order)
        nt = B.n_terms(c)
        assert (nt["bonds"], nt["angles"], nt["torsions"]) == (70, 65, 130) and np.all(c.charge != 0) and abs(c.charge.sum()) < 1e-4
        assert run_ratio(c, np.float32).max() <= 1.01 * YARD32_RUN[f"small_o{order}"]


if __name__ == "__main__":
    print("ORACLE_VS_EWALD = {")
    for w in ("orthorhombic", "sheared", "net_charge"):
        print(f'    "{w}": ({", ".join(f"{v:.2e}" for v in oracle_vs_ewald(w))}),')
    print("}\nCONVERGENCE = {")
    for o in (4, 5, 6):
        print(f'    {o}: ({", ".join(f"{v:.2e}" for v in oracle_vs_ewald("orthorhombic", o, COARSE))}),')
    print("}\nYARD32_RUN = {")
    for k, v in measure_run().items():
        print(f'    "{k}": {v:.2e},')
    print("}")
