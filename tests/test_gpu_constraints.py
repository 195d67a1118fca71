"""SHAKE_RATTLE in the device step loops (csrc/constraints.hip, mhip_set_constraints) against the fp64 numpy restatement of
tests/constraints_ref.py: VV and Langevin on 6mrr with H-bond constraints and rigid water, every cluster kind on a toy system, the
fp32 PME run holding its 15 380 constraints, chunked continuation, removal, and every refusal of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from tests import constraints_ref as R
from tests import systems as S  # noqa: F401  (Case.oracle)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -6


def sixmrr(dtype=np.float64, coulomb="rf", pme=False):
    from molly_jl_amd.workloads import protein_6mrr
    return protein_6mrr(coulomb=coulomb, dtype=dtype, pme=pme, constraints="hbonds", rigid_water=True)


def set_tol(case, tol, max_iters=25):
    case.constraints = dict(case.constraints, dist_tolerance=tol, max_iters=max_iters)
    return case


def dev(a, b, box):
    return float(np.abs(R.min_image(np.asarray(a, np.float64) - np.asarray(b, np.float64), box)).max())


def draws(seed, n):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(n)]


def test_6mrr_velocity_verlet_2fs_matches_the_reference(pkg, slack):
    case = set_tol(sixmrr(), 1e-10)
    cons = R.of_case(case, tol=1e-10)
    s = case.system(pkg, np.float64)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002, remove_CM_motion=1), 20)
    x, v = R.vv_run(case.oracle(np.float64), cons, case.coords, case.velocities, 20, 0.002, remove_cm_every=1)
    info = s.constraint_info()
    assert (info["clusters12"], info["clusters23"], info["clusters34"], info["angle_clusters"], info["n_constraints"]) == (186, 133, 48, 4928, 15380)
    assert info["n_not_converged"] == 0 and info["max_iters_last_run"] >= 1
    # bars: 3x the deviations measured on an MI355X (7.4e-11 nm, 6.0e-9 nm/ps, 9.8e-11 nm)
    slack("coords vs numpy reference (nm)", dev(s.coords, x, case.box), 2.2e-10)
    slack("velocities vs numpy reference (nm/ps)", float(np.abs(s.velocities - v).max()), 1.8e-8)
    e_d, e_v = cons.check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
    slack("constraint lengths (nm)", e_d, 3e-10)


def test_6mrr_langevin_2fs_matches_the_reference(pkg, slack):
    case = set_tol(sixmrr(), 1e-10)
    cons = R.of_case(case, tol=1e-10)
    s = case.system(pkg, np.float64)
    key, ctr1 = draws(17, 2)
    pkg.simulate(s, pkg.Langevin(dt=0.002, temperature=300.0, friction=1.0), 10, rng=17)
    x, v = R.langevin_run(case.oracle(np.float64), cons, case.coords, case.velocities, 10, 0.002, 8.314462618e-3 * 300.0, 1.0, key, ctr1)
    # bars: 3x the deviations measured on an MI355X (4.8e-11 nm, 3.9e-8 nm/ps)
    slack("coords vs numpy reference (nm)", dev(s.coords, x, case.box), 1.5e-10)
    slack("velocities vs numpy reference (nm/ps)", float(np.abs(s.velocities - v).max()), 1.2e-7)


@pytest.mark.parametrize("integrator", ["vv", "langevin"])
def test_every_cluster_kind_on_a_toy_system(pkg, slack, integrator):
    case = set_tol(R.toy_system(), 1e-10)
    cons = R.of_case(case, tol=1e-10)
    assert {k: len(v[0]) for k, v in cons.clusters.items()} == {"2": 16, "3": 16, "4": 16, "angle": 16}
    s = case.system(pkg, np.float64)
    o = case.oracle(np.float64)
    if integrator == "vv":
        pkg.simulate(s, pkg.VelocityVerlet(dt=0.002, remove_CM_motion=5), 50)
        x, v = R.vv_run(o, cons, case.coords, case.velocities, 50, 0.002, remove_cm_every=5)
    else:
        key, ctr1 = draws(4, 2)
        pkg.simulate(s, pkg.Langevin(dt=0.002, temperature=300.0, friction=2.0, remove_CM_motion=5), 50, rng=4)
        x, v = R.langevin_run(o, cons, case.coords, case.velocities, 50, 0.002, 8.314462618e-3 * 300.0, 2.0, key, ctr1, remove_cm_every=5)
    # bars: 3x the deviations measured on an MI355X (VV: 1.4e-11 nm, 1.4e-10 nm/ps, 8.5e-12 nm, 3.8e-16 nm/ps; Langevin: 9.9e-12 nm, 1.4e-9 nm/ps, 9.6e-11 nm)
    bars = dict(vv=(4.2e-11, 4.5e-10, 2.6e-11), langevin=(3e-11, 4.3e-9, 2.9e-10))[integrator]
    slack("coords vs numpy reference (nm)", dev(s.coords, x, case.box), bars[0])
    slack("velocities vs numpy reference (nm/ps)", float(np.abs(s.velocities - v).max()), bars[1])
    e_d, e_v = cons.check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
    slack("constraint lengths (nm)", e_d, bars[2])
    if integrator == "vv":      # (a Langevin step ends with SHAKE's velocity correction, not with RATTLE: its v_ij · r_ij is not zero, the reference's neither)
        slack("v_ij . r_ij / |r_ij| (nm/ps)", e_v, 1.2e-15)


def test_6mrr_fp32_pme_holds_every_constraint_for_1000_steps(pkg, slack):
    case = sixmrr(np.float32, coulomb="ewald", pme=True)
    cons = R.of_case(case, tol=1e-8)
    s = case.system(pkg, np.float32)
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=1)
    worst_d = worst_v = 0.0
    energies = []
    for chunk in range(10):
        pkg.simulate(s, sim, 100, init_step=100 * chunk)
        e_d, e_v = cons.check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
        worst_d, worst_v = max(worst_d, e_d), max(worst_v, e_v)
        energies.append(pkg.total_energy(s))
    # the drift from the end of the first chunk: the first SHAKE snaps the flexible start onto the constraints (its velocity correction
    # heats the system once), after that the constrained NVE run conserves energy
    drift = abs(energies[-1] - energies[0])
    print(f"total energy per chunk (kJ/mol): {[round(e, 1) for e in energies]}, temperature {pkg.temperature(s):.1f} K")
    info = s.constraint_info()
    assert info["n_constraints"] == 15380 and info["n_not_converged"] == 0
    slack("constraint lengths over 1000 steps (nm)", worst_d, 1e-5)
    slack("v_ij . r_ij / |r_ij| over 1000 steps (nm/ps)", worst_v, 3.5e-5)      # (3x the 1.1e-5 measured)
    slack("NVE total-energy drift from step 100 to 1000 (kJ/mol)", drift, 45.0)      # (3x the 15 kJ/mol measured on an MI355X, of 122 650)


def _raw_run(pkg, case, dtype, runs, langevin, device):
    """runs: list of (first, n) chunks; state in and out through host or device (torch) pointers"""
    L = pkg.lib()
    s = case.system(pkg, dtype)
    s.push_state(velocities=True)
    if device:
        import torch
        td = torch.float32 if dtype == np.float32 else torch.float64
        xd = torch.tensor(s.coords, dtype=td, device="cuda"); vd = torch.tensor(s.velocities, dtype=td, device="cuda")
        torch.cuda.synchronize()
        assert L.mhip_set_state(s._ctx, C.c_void_p(xd.data_ptr()), C.c_void_p(vd.data_ptr()), 1) == 0
    for first, n in runs:
        if langevin:
            rc = L.mhip_langevin_run(s._ctx, first, n, 0.002, 2.494, 1.0, 0, 11, 1000 + first)
        else:
            rc = L.mhip_vv_run(s._ctx, first, n, 0.002, 0)
        assert rc == 0, L.mhip_last_error(s._ctx).decode()
    if device:
        assert L.mhip_get_state(s._ctx, C.c_void_p(xd.data_ptr()), C.c_void_p(vd.data_ptr()), 1) == 0
        torch.cuda.synchronize()
        return xd.cpu().numpy(), vd.cpu().numpy(), s.stats()["n_fused_steps"]
    s.pull_state()
    return s.coords.copy(), s.velocities.copy(), s.stats()["n_fused_steps"]


@pytest.mark.parametrize("langevin", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_chunked_runs_continue_bit_for_bit(pkg, langevin, device):
    """reaction field: no atomics on the force path (the PME mesh is flushed with float atomics and repeats to rounding only)"""
    case = sixmrr(np.float32, coulomb="rf")
    x1, v1, _ = _raw_run(pkg, case, np.float32, [(0, 100)], langevin, device)
    x2, v2, _ = _raw_run(pkg, case, np.float32, [(0, 50), (50, 50)], langevin, device)
    assert np.array_equal(x1, x2) and np.array_equal(v1, v2)


@pytest.mark.parametrize("langevin", [False, True])
def test_removed_constraints_run_as_never_constrained(pkg, langevin):
    """the fp32 one-type fluid, whose pair pass integrates in its epilogue (n_fused_steps > 0): after the removal it does so again"""
    case = S.lj_fluid(40, seed=2, dtype=np.float32)      # 64 000 atoms: the packed loop that integrates in its epilogue
    x0, v0, f0 = _raw_run(pkg, case, np.float32, [(0, 60)], langevin, False)
    L = pkg.lib()
    s = case.system(pkg, np.float32)
    s.push_state(velocities=True)
    i = np.array([0], np.int32); j = np.array([1], np.int32); d = np.array([0.1])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mhip_set_constraints(s._ctx, 1, p(i), p(j), p(d), 0, None, None, None, None, 1e-8, 1e-8, 25) == 0
    assert L.mhip_set_constraints(s._ctx, 0, None, None, None, 0, None, None, None, None, 1e-8, 1e-8, 25) == 0
    rc = L.mhip_langevin_run(s._ctx, 0, 60, 0.002, 2.494, 1.0, 0, 11, 1000) if langevin else L.mhip_vv_run(s._ctx, 0, 60, 0.002, 0)
    assert rc == 0
    s.pull_state()
    assert np.array_equal(s.coords, x0) and np.array_equal(s.velocities, v0)
    assert s.stats()["n_fused_steps"] == f0 and f0 > 0


def test_refusals(pkg):
    from molly_jl_amd.workloads import protein_6mrr
    L = pkg.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    i32 = lambda *a: np.array(a, np.int32)
    f64 = lambda *a: np.array(a, np.float64)

    def fresh():
        s = R.toy_system().system(pkg, np.float64)
        s.constraints = ()
        s.push_state(velocities=True)
        return s

    def setc(s, dist=None, angle=None):
        di, dj, dd = dist if dist else (None, None, None)
        ai, aj, ak, d3 = angle if angle else (None, None, None, None)
        return L.mhip_set_constraints(s._ctx, 0 if dist is None else len(di), p(di), p(dj), p(dd), 0 if angle is None else len(ai),
                                      p(ai), p(aj), p(ak), p(d3), 1e-8, 1e-8, 25)
    s = fresh()
    invalid = {
        "chain": ((i32(0, 1, 2), i32(1, 2, 3), f64(.1, .1, .1)), None),
        "ring": ((i32(0, 1, 2), i32(1, 2, 0), f64(.1, .1, .1)), None),
        "four on one centre": ((i32(0, 0, 0, 0), i32(1, 2, 3, 4), f64(.1, .1, .1, .1)), None),
        "atom in two clusters": ((i32(0), i32(1), f64(.1)), (i32(1), i32(2), i32(3), f64(.1, .1, .15))),
        "linear angle": (None, (i32(0), i32(1), i32(2), f64(.1, .1, .2))),
        "index out of range": ((i32(0), i32(len(s)), f64(.1)), None),
    }
    for what, (dist, angle) in invalid.items():
        assert setc(s, dist, angle) == ERR_INVALID, what
    ok = ((i32(0), i32(1), f64(.1)), None)
    # Andersen coupling and constraints, either order
    assert L.mhip_set_andersen(s._ctx, 2.494, 0.1, 3) == 0
    assert setc(s, *ok) == ERR_UNSUPPORTED
    assert L.mhip_set_andersen(s._ctx, 0.0, 0.0, 0) == 0
    assert setc(s, *ok) == 0
    assert L.mhip_set_andersen(s._ctx, 2.494, 0.1, 3) == ERR_UNSUPPORTED
    # the split step and ghosts
    assert L.mhip_vv_init(s._ctx, 0) == ERR_UNSUPPORTED
    assert L.mhip_vv_stage1(s._ctx, 0.002) == ERR_UNSUPPORTED
    assert L.mhip_vv_stage2(s._ctx, 1, 0.002) == ERR_UNSUPPORTED
    assert L.mhip_set_atom_counts(s._ctx, len(s) - 4, 4) == ERR_UNSUPPORTED
    # TriclinicBoundary, either order
    bv = np.diag(s.boundary.side_lengths).astype(np.float64).reshape(-1)
    assert L.mhip_set_triclinic(s._ctx, p(bv), 1) == ERR_UNSUPPORTED
    s2 = fresh()
    assert L.mhip_set_triclinic(s2._ctx, p(bv), 1) == 0
    assert setc(s2, *ok) == ERR_UNSUPPORTED
    # contexts with ghosts
    s3 = fresh()
    assert L.mhip_set_atom_counts(s3._ctx, len(s3) - 4, 4) == 0
    assert setc(s3, *ok) == ERR_UNSUPPORTED
    # the Python mirror: virial / pressure / minimiser / barostat refuse a constrained System
    c = protein_6mrr(coulomb="rf", constraints="hbonds")
    sc = c.system(pkg, np.float32)
    for f in (lambda: pkg.virial(sc), lambda: pkg.pressure(sc), lambda: pkg.simulate(sc, pkg.SteepestDescentMinimizer())):
        with pytest.raises(pkg.MollyHipError):
            f()
    baro = pkg.MonteCarloBarostat(1.0, 300.0, sc.boundary)
    with pytest.raises(pkg.MollyHipError):
        pkg.simulate(sc, pkg.Langevin(dt=0.002, temperature=300.0, friction=1.0, coupling=baro), 10)
    # temperature counts 3N − 3 − n_constraints degrees of freedom
    # (H-bonds without rigid water: the protein's 596 and both O-H bonds of every water)
    ke = pkg.kinetic_energy(sc)
    assert sc.n_constraints == 596 + 2 * 4928
    assert abs(pkg.temperature(sc) - 2 * ke / ((3 * len(sc) - 3 - sc.n_constraints) * pkg.BOLTZMANN)) < 1e-9 * pkg.temperature(sc)
