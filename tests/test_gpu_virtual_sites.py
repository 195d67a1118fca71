"""Virtual sites on the device (csrc/virtual_sites.hip, the hosted sites of csrc/constraints.hip, mhip_set_virtual_sites) against the fp64
numpy restatement of tests/virtual_sites_ref.py: the reference's known answers through the C ABI, VV and Langevin trajectories of rigid
and flexible four-site water and of the reference's toy system, the fp32 PME box over 1 000 steps, chunked continuation, removal, every
refusal, and the dispatch count of a step."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import constraints_ref as CR
from tests import systems as S
from tests import virtual_sites_ref as V

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -6
KB = 8.314462618e-3
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def dev(a, b, box):
    return float(np.abs(CR.min_image(np.asarray(a, np.float64) - np.asarray(b, np.float64), box)).max())


def draws(seed, n):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(n)]


def set_sites(L, s, sites):
    t, a, a1, a2, a3, w = V.site_arrays(sites)
    return L.mhip_set_virtual_sites(s._ctx, len(t), p(t), p(a), p(a1), p(a2), p(a3), p(w))


def info(L, s):
    out = (C.c_int64 * 8)()
    assert L.mhip_virtual_site_info(s._ctx, C.byref(out)) == 0
    return list(out)


# ---- 4. known answers -------------------------------------------------------------------------------------------------------------------
def test_known_answers_fp64(pkg, slack):
    """the reference's toy: every pair interacts (no cutoff, no list) except the excluded one, whose atoms coincide"""
    L = pkg.lib()
    g = V.toy()
    case = V.toy_case(g)
    s = case.system(pkg, np.float64, coords=g["coords"])
    pkg.place_virtual_sites(s)
    slack("placed coordinates (nm)", np.linalg.norm(s.coords - g["coords_true"], axis=1).max(), 1e-10)
    assert s.virtual_site_info() == dict(one_particle=1, two_particle=2, three_particle=1, out_of_plane=1, n_hosted=5, n_host_items=3, n_groups=3)
    # the spread alone: the numpy raw forces through mhip_distribute_forces, host and device pointers
    # (at numpy's own placement, as the known answers were made: the rounded literals of coords_true are 1e-15 nm away, which this stiff toy — gradients of
    # 1e6 kJ/mol/nm² between sites 0.064 nm apart — turns into 1e-9 kJ/mol/nm)
    raw, _ = V.lj_all_pairs(V.place(g["coords"], g["box"], g["sites"]), g["box"], g["sigma"], g["eps"], g["excluded"])
    f = raw.copy()
    assert L.mhip_distribute_forces(s._ctx, p(f), 0) == 0
    slack("distributed numpy forces, host pointer (kJ/mol/nm)", np.linalg.norm(f - g["fs_true"], axis=1).max(), 1e-9)
    import torch
    fd = torch.tensor(raw, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.mhip_distribute_forces(s._ctx, C.c_void_p(fd.data_ptr()), 1) == 0
    assert L.mhip_synchronize(s._ctx) == 0
    slack("distributed numpy forces, device pointer (kJ/mol/nm)", np.linalg.norm(fd.cpu().numpy() - g["fs_true"], axis=1).max(), 1e-9)
    # end to end: the engine's raw forces first (r_list = +inf with an exclusion), then forces(sys)
    raw_e = np.zeros_like(raw)
    assert L.mhip_forces(s._ctx, 0, 0, p(raw_e), None, 0) == 0, L.mhip_last_error(s._ctx).decode()
    d_raw = float(np.linalg.norm(raw_e - raw, axis=1).max())
    print(f"raw engine forces against numpy: {d_raw:.3e}")
    fs = pkg.forces(s)
    slack("forces(sys) against fs_true (kJ/mol/nm)", np.linalg.norm(fs - g["fs_true"], axis=1).max(), 1e-9 + 4 * d_raw)
    assert np.linalg.norm(fs.sum(0)) < 1e-9 + 4 * d_raw * math.sqrt(len(fs))
    assert not fs[g["flags"]].any()
    # random_velocities!: exactly the sites stay at zero
    pkg.random_velocities(s, 300.0, rng=3)
    moving = np.any(s.velocities != 0, axis=1)
    assert np.array_equal(moving, ~g["flags"])
    # temperature: 3 (N − n_sites) − 3 degrees of freedom
    assert pkg.temperature(s) == pytest.approx(2 * pkg.kinetic_energy(s) / ((3 * 8 - 3) * pkg.BOLTZMANN), rel=1e-12)


def test_remove_cm_leaves_site_velocities_alone(pkg):
    g = V.toy()
    rng = np.random.default_rng(5)
    v = rng.normal(size=(13, 3)) + 2.0
    s = V.toy_case(g).system(pkg, np.float64, velocities=v)
    pkg.remove_CM_motion(s)
    m = g["mass"]
    assert np.array_equal(s.velocities[g["flags"]], v[g["flags"]])
    vcm = (m[:, None] * v).sum(0) / m.sum()
    assert np.abs(s.velocities[~g["flags"]] - (v[~g["flags"]] - vcm)).max() < 1e-14


def test_velocity_draws_go_by_the_site_flags(pkg):
    """sites that carry a mass (accepted outside the step loops): the flags decide, not m = 0 — random_velocities! zeroes them, the Andersen re-draw
    and the centre-of-mass removal leave them alone (spatial.jl:823-831, 926; coupling.jl:209)"""
    g = V.toy()
    case = V.toy_case(g)
    case.mass = np.full(13, 10.0)
    s = case.system(pkg, np.float64, velocities=np.full((13, 3), 1.5))
    pkg.random_velocities(s, 300.0, rng=3)
    assert not s.velocities[g["flags"]].any() and np.all(np.any(s.velocities[~g["flags"]] != 0, axis=1))
    s.velocities[g["flags"]] = 1.5
    before = s.velocities.copy()
    pkg.apply_coupling(s, pkg.AndersenThermostat(300.0, 0.001), pkg.VelocityVerlet(dt=0.001), rng=4)      # probability dt / coupling_const = 1
    assert np.array_equal(s.velocities[g["flags"]], before[g["flags"]])
    assert np.all(np.any(s.velocities[~g["flags"]] != before[~g["flags"]], axis=1))
    pkg.remove_CM_motion(s)
    assert np.array_equal(s.velocities[g["flags"]], before[g["flags"]])


# ---- 5. trajectories --------------------------------------------------------------------------------------------------------------------
# velocity bars: 3x the deviation of the THREE-site version of the same box (M removed, its charge on O) from constraints_ref over the same
# steps, measured on an MI355X with the library of commit ed82a24 (before sites): rigid VV 1.64e-12, rigid Langevin 1.04e-12, flexible VV
# 6.46e-13, flexible Langevin 6.96e-13 nm/ps
VEL_BAR = {(True, "vv"): 3 * 1.64e-12, (True, "langevin"): 3 * 1.04e-12, (False, "vv"): 3 * 6.46e-13, (False, "langevin"): 3 * 6.96e-13}


def _run_both(pkg, case, cons, force_fn, randn3, integ, n, dt, cm):
    s = case.system(pkg, np.float64)
    if integ == "vv":
        pkg.simulate(s, pkg.VelocityVerlet(dt=dt, remove_CM_motion=cm), n)
        x, v = V.vv_run(force_fn, cons, case.virtual_sites, case.coords, case.velocities, case.mass, case.box, n, dt, remove_cm_every=cm)
    else:
        key, ctr1 = draws(17, 2)
        pkg.simulate(s, pkg.Langevin(dt=dt, temperature=300.0, friction=1.0, remove_CM_motion=cm), n, rng=17)
        x, v = V.langevin_run(force_fn, cons, case.virtual_sites, case.coords, case.velocities, case.mass, case.box, n, dt, KB * 300.0, 1.0, key, ctr1,
                              randn3, remove_cm_every=cm)
    return s, x, v


@pytest.mark.parametrize("integ", ["vv", "langevin"])
@pytest.mark.parametrize("rigid", [True, False])
def test_four_site_water_matches_the_reference(pkg, slack, rigid, integ):
    case = V.tip4p_box(8, rigid=rigid)
    assert case.n == 2048
    cons = None
    if rigid:
        case.constraints = dict(case.constraints, dist_tolerance=1e-10, max_iters=25)
        cons = CR.of_case(case, tol=1e-10)
    o = case.oracle(np.float64)
    s, x, v = _run_both(pkg, case, cons, V.oracle_forces(o), o.randn3, integ, 20, 0.002 if rigid else 0.0005, 1)
    slack("coords vs numpy reference (nm)", dev(s.coords, x, case.box), 1e-9)
    slack("velocities vs numpy reference (nm/ps)", float(np.abs(s.velocities - v).max()), VEL_BAR[(rigid, integ)])
    xs = s.coords.astype(np.float64)
    slack("sites on place(parents) (nm)", dev(xs, V.place(xs, case.box, case.virtual_sites), case.box), 1e-12)
    assert not s.velocities[3::4].any()
    vi = s.virtual_site_info()
    if rigid:
        e_d, _ = cons.check(xs, s.velocities.astype(np.float64))
        slack("constraint lengths (nm)", e_d, 3e-10)
        ci = s.constraint_info()
        assert ci["angle_clusters"] == 512 and ci["n_not_converged"] == 0
        assert (vi["n_hosted"], vi["n_host_items"], vi["n_groups"]) == (512, 512, 0)      # all hosted, items = waters
    else:
        assert (vi["n_hosted"], vi["n_host_items"], vi["n_groups"]) == (512, 512, 512)


@pytest.mark.parametrize("integ", ["vv", "langevin"])
def test_toy_system_matches_the_reference(pkg, slack, integ):
    """unconstrained groups, two sites on one group, an out-of-plane site, a one-particle site; forces up to 9.4e3 kJ/mol/nm"""
    g = V.toy()
    case = V.toy_case(g)
    o = case.oracle(np.float64)
    force_fn = lambda x: V.lj_all_pairs(x, g["box"], g["sigma"], g["eps"], g["excluded"])[0]
    s, x, v = _run_both(pkg, case, None, force_fn, o.randn3, integ, 50, 0.0005, 1)
    slack("coords vs numpy reference (nm)", dev(s.coords, x, case.box), 1e-9)
    slack("velocities vs numpy reference (nm/ps)", float(np.abs(s.velocities - v).max()), VEL_BAR[(False, integ)])
    xs = s.coords.astype(np.float64)
    slack("sites on place(parents) (nm)", dev(xs, V.place(xs, case.box, case.virtual_sites), case.box), 1e-12)
    assert not s.velocities[g["flags"]].any()


# ---- 6. fp32 ----------------------------------------------------------------------------------------------------------------------------
def _rounded(case):
    for k in ("coords", "charge", "sigma", "eps", "mass"):
        setattr(case, k, np.asarray(getattr(case, k), dtype=np.float32).astype(np.float64))
    return case


def test_fp32_distributed_forces_pme(pkg, slack):
    """the pair part at the project's fp32 bar, where a parent's scale is its own plus Σ|w| of its sites' scales (the distribution is linear);
    the mesh part at the bar of the 6mrr PME test (5e-5 of the largest reciprocal-space force + 2.5e-4)"""
    case = _rounded(V.tip4p_box(12, coulomb="pme"))
    tol, o, nl = S.fp32_force_tolerance(case)
    sites = case.virtual_sites
    absw = [(v[0], v[1], v[2], v[3], v[4], *[abs(w) for w in v[5:]]) for v in sites]
    bar = V.distribute(np.repeat(tol[:, None], 3, axis=1), case.coords, case.box, absw)[:, 0]
    s = case.system(pkg, np.float32)
    f_pair = o.forces(nl, nthreads=8, specific=True)              # (specific: the Ewald exclusion terms of the intramolecular pairs)
    f_ref = V.distribute(f_pair, case.coords, case.box, sites)
    f = pkg.forces(s, general=False).astype(np.float64)
    err = np.linalg.norm(f - f_ref, axis=1)
    parents = ~V.flags(case.n, sites)
    assert not f[~parents].any()
    S.fp32_check(err[parents], bar[parents], "fp32 distributed pair forces against the fp64 reference")
    g_ref = o.forces(None, pairwise=False, specific=False, general=True)
    pme_scale = np.linalg.norm(g_ref, axis=1).max()
    f_all = pkg.forces(s).astype(np.float64)
    err = np.linalg.norm(f_all - V.distribute(f_pair + g_ref, case.coords, case.box, sites), axis=1)
    mesh = V.distribute(np.full((case.n, 3), 5e-5 * pme_scale + 2.5e-4), case.coords, case.box, absw)[:, 0]
    slack("fp32 distributed total forces (pair + PME): worst error / bar", (err[parents] / (bar + mesh)[parents]).max(), 1.0)


def test_fp32_pme_1000_steps(pkg, slack):
    case = V.tip4p_box(12, coulomb="pme")
    cons = CR.of_case(case, tol=1e-8)
    s = case.system(pkg, np.float32)
    L = pkg.lib()
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=1)
    worst = 0.0
    for chunk in range(10):
        pkg.simulate(s, sim, 100, init_step=100 * chunk, check_nans=True)
        xs = s.coords.astype(np.float64)
        worst = max(worst, dev(xs, V.place(xs, case.box, case.virtual_sites), case.box))
    assert s.constraint_info()["n_not_converged"] == 0
    # fp32 rounding of a coordinate below 3.72 nm: half an ulp is 1.2e-7; the site is a sum of four rounded terms
    slack("sites on place(parents) over 1000 steps (nm)", worst, 4 * 1.2e-7)
    e_d, _ = cons.check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
    slack("constraint lengths (nm)", e_d, 1e-5)
    # the list the run ends with covers what a fresh context finds at the same coordinates (a site missing from the displacement check would not)
    keys, _ = S.export_keys(pkg, s)
    s2 = case.system(pkg, np.float32, coords=s.coords, velocities=s.velocities)
    s2.push_state(velocities=True)
    keys2, _ = S.export_keys(pkg, s2)
    assert np.array_equal(keys, keys2)
    print(f"temperature after 1000 steps: {pkg.temperature(s):.1f} K")


# ---- 7. chunks, removal ---------------------------------------------------------------------------------------------------------------
def _raw_run(pkg, case, dtype, runs, langevin, device):
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
        rc = L.mhip_langevin_run(s._ctx, first, n, 0.002, 2.494, 1.0, 0, 11, 1000 + first) if langevin else L.mhip_vv_run(s._ctx, first, n, 0.002, 0)
        assert rc == 0, L.mhip_last_error(s._ctx).decode()
        if device:      # hand the state back between chunks, as a caller that keeps it on the device does
            assert L.mhip_get_state(s._ctx, C.c_void_p(xd.data_ptr()), C.c_void_p(vd.data_ptr()), 1) == 0
            assert L.mhip_set_state(s._ctx, C.c_void_p(xd.data_ptr()), C.c_void_p(vd.data_ptr()), 1) == 0
        else:
            s.pull_state(); s.push_state(velocities=True)
    if device:
        torch.cuda.synchronize()
        return xd.cpu().numpy(), vd.cpu().numpy(), s.stats()["n_fused_steps"]
    return s.coords.copy(), s.velocities.copy(), s.stats()["n_fused_steps"]


@pytest.mark.parametrize("langevin", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_chunked_runs_continue_bit_for_bit(pkg, langevin, device):
    case = V.tip4p_box(12, coulomb="rf")
    x1, v1, _ = _raw_run(pkg, case, np.float32, [(0, 100)], langevin, device)
    x2, v2, _ = _raw_run(pkg, case, np.float32, [(0, 50), (50, 50)], langevin, device)
    assert np.array_equal(x1, x2) and np.array_equal(v1, v2)


@pytest.mark.parametrize("langevin", [False, True])
def test_removed_sites_run_as_never_set(pkg, langevin):
    case = S.lj_fluid(40, seed=2, dtype=np.float32)      # 64 000 atoms: the packed loop that integrates in its epilogue
    x0, v0, f0 = _raw_run(pkg, case, np.float32, [(0, 60)], langevin, False)
    L = pkg.lib()
    s = case.system(pkg, np.float32)
    s.push_state(velocities=True)
    assert set_sites(L, s, [(2, 5, 0, 1, -1, 0.5, 0.5, 0, 0, 0, 0)]) == 0
    assert info(L, s)[:7] == [0, 1, 0, 0, 1, 1, 1]
    assert L.mhip_set_virtual_sites(s._ctx, 0, None, None, None, None, None, None) == 0
    assert info(L, s)[:7] == [0] * 7
    rc = L.mhip_langevin_run(s._ctx, 0, 60, 0.002, 2.494, 1.0, 0, 11, 1000) if langevin else L.mhip_vv_run(s._ctx, 0, 60, 0.002, 0)
    assert rc == 0
    s.pull_state()
    assert np.array_equal(s.coords, x0) and np.array_equal(s.velocities, v0)
    assert s.stats()["n_fused_steps"] == f0 and f0 > 0


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    L = pkg.lib()
    i32 = lambda *a: np.array(a, np.int32)
    f64 = lambda *a: np.array(a, np.float64)

    def fresh(mass0=(3,)):
        case = CR.toy_system()
        case.mass = case.mass.copy(); case.mass[list(mass0)] = 0.0
        s = case.system(pkg, np.float64)
        s.constraints = ()
        s.push_state(velocities=True)
        return s
    n = len(fresh())
    one = lambda site, a1: (1, site, a1, -1, -1, 0, 0, 0, 0, 0, 0)
    s = fresh()
    invalid = {
        "type": [(5, 3, 0, -1, -1, 0, 0, 0, 0, 0, 0)],
        "site out of range": [one(n, 0)],
        "parent out of range": [one(3, n)],
        "defined twice": [one(3, 0), one(3, 1)],
        "parent is a site": [one(3, 0), one(4, 3)],
        "weights of two": [(2, 3, 0, 1, -1, 0.6, 0.5, 0, 0, 0, 0)],
        "weights of three": [(3, 3, 0, 1, 2, 0.3, 0.3, 0.5, 0, 0, 0)],
    }
    for what, sites in invalid.items():
        assert set_sites(L, s, sites) == ERR_INVALID, what
    assert set_sites(L, s, [(2, 3, 0, 1, -1, 0.6, 0.4 + 1e-10, 0, 0, 0, 0)]) == 0       # within isapprox
    # a site in a constraint, either order
    cst = lambda s, i, j: L.mhip_set_constraints(s._ctx, 1, p(i32(i)), p(i32(j)), p(f64(0.1)), 0, None, None, None, None, 1e-8, 1e-8, 25)
    assert cst(s, 3, 8) == ERR_INVALID
    assert cst(s, 8, 9) == 0
    assert set_sites(L, s, [one(9, 0)]) == ERR_INVALID
    assert info(L, s)[1] == 1                                  # a refused set leaves the one before in place
    # the Andersen coupling, either order
    assert L.mhip_set_andersen(s._ctx, 2.494, 0.1, 3) == ERR_UNSUPPORTED
    s1 = fresh()
    assert L.mhip_set_andersen(s1._ctx, 2.494, 0.1, 3) == 0
    assert set_sites(L, s1, [one(3, 0)]) == ERR_UNSUPPORTED
    # the split step, ghosts
    assert L.mhip_vv_init(s._ctx, 0) == ERR_UNSUPPORTED
    assert L.mhip_vv_stage1(s._ctx, 0.002) == ERR_UNSUPPORTED
    assert L.mhip_vv_stage2(s._ctx, 1, 0.002) == ERR_UNSUPPORTED
    assert L.mhip_set_atom_counts(s._ctx, n - 4, 4) == ERR_UNSUPPORTED
    s3 = fresh()
    assert L.mhip_set_atom_counts(s3._ctx, n - 4, 4) == 0
    assert set_sites(L, s3, [one(3, 0)]) == ERR_UNSUPPORTED
    # TriclinicBoundary, either order
    bv = np.diag(s.boundary.side_lengths).astype(np.float64).reshape(-1)
    assert L.mhip_set_triclinic(s._ctx, p(bv), 1) == ERR_UNSUPPORTED
    s2 = fresh()
    assert L.mhip_set_triclinic(s2._ctx, p(bv), 1) == 0
    assert set_sites(L, s2, [one(3, 0)]) == ERR_UNSUPPORTED
    # a site with a mass: accepted by the setter, refused when a run starts; set-then-remove leaves no trace
    s4 = fresh(mass0=())
    assert set_sites(L, s4, [one(3, 0)]) == 0
    assert L.mhip_vv_run(s4._ctx, 0, 2, 0.001, 0) == ERR_INVALID
    assert L.mhip_langevin_run(s4._ctx, 0, 2, 0.001, 2.494, 1.0, 0, 11, 0) == ERR_INVALID
    assert b"mass" in L.mhip_last_error(s4._ctx)
    assert L.mhip_set_virtual_sites(s4._ctx, 0, None, None, None, None, None, None) == 0
    assert L.mhip_vv_run(s4._ctx, 0, 2, 0.001, 0) == 0
    # a set no single item can host: accepted (the one-shot calls serve it), the runs refuse it and name the site
    s5 = fresh(mass0=(3, 12))
    ang = (i32(5), i32(4), i32(6), f64(0.1, 0.1, 0.15))
    assert L.mhip_set_constraints(s5._ctx, 1, p(i32(8)), p(i32(9)), p(f64(0.1)), 1, p(ang[0]), p(ang[1]), p(ang[2]), p(ang[3]), 1e-8, 1e-8, 25) == 0
    assert set_sites(L, s5, [one(3, 0), (2, 12, 8, 4, -1, 0.5, 0.5, 0, 0, 0, 0)]) == 0
    v = info(L, s5)
    assert v[0] + v[1] == 2 and v[4] == 1                      # hosted < total
    assert L.mhip_place_virtual_sites(s5._ctx) == 0
    assert L.mhip_vv_run(s5._ctx, 0, 2, 0.001, 0) == ERR_UNSUPPORTED
    assert b"site 1" in L.mhip_last_error(s5._ctx)
    assert L.mhip_langevin_run(s5._ctx, 0, 2, 0.001, 2.494, 1.0, 0, 11, 0) == ERR_UNSUPPORTED
    # … and a union of free parents above four atoms
    s6 = fresh(mass0=(3, 12, 13))
    sites = [(3, 3, 0, 1, 2, 0.4, 0.3, 0.3, 0, 0, 0), (3, 12, 2, 16, 17, 0.4, 0.3, 0.3, 0, 0, 0)]
    assert set_sites(L, s6, sites) == 0
    assert info(L, s6)[4] == 0
    assert L.mhip_vv_run(s6._ctx, 0, 2, 0.001, 0) == ERR_UNSUPPORTED


# ---- 9. no added dispatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("langevin", [False, True])
def test_no_added_dispatch_per_step(pkg, langevin):
    """with profiling on, the integrator stage (prof_calls[2]) of the rigid four-site box is launched as often as that of its three-site version"""
    L = pkg.lib()
    calls = []
    for three in (False, True):
        case = V.tip4p_box(12, coulomb="pme", three_site=three)
        s = case.system(pkg, np.float32)
        s.push_state(velocities=True)
        assert L.mhip_set_profiling(s._ctx, 1) == 0
        rc = L.mhip_langevin_run(s._ctx, 0, 200, 0.002, 2.494, 1.0, 1, 11, 1000) if langevin else L.mhip_vv_run(s._ctx, 0, 200, 0.002, 1)
        assert rc == 0, L.mhip_last_error(s._ctx).decode()
        calls.append(s.stats()["prof_calls"][2])
    assert calls[0] == calls[1] and calls[0] in (200, 201)


def test_no_site_kernel_between_the_steps_of_a_run(tmp_path):
    """the kernel names of a `rocprofv3 --kernel-trace --stats` run of tools/micro/tip4p_water.py (a child process of its own): the sites are placed once where a
    run starts from coordinates handed in (every simulate call of the tool's four-site halves: three per integrator) and served by k_con_step from then on"""
    import csv
    import glob
    import os
    import shutil
    import subprocess
    import sys
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        pytest.skip("rocprofv3 not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tmp_path), "--", sys.executable,
                        os.path.join(root, "tools", "micro", "tip4p_water.py"), "8", "100"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_trace.csv"), recursive=True)
    assert files, os.listdir(str(tmp_path))
    names = [row["Kernel_Name"] for f in files for row in csv.DictReader(open(f))]
    n_place = sum("k_vs_place" in n for n in names)
    n_spread = sum("k_vs_spread" in n for n in names)
    n_step = sum("k_con_step" in n for n in names)
    print(f"k_vs_place {n_place}, k_vs_spread {n_spread}, k_con_step {n_step} of {len(names)} dispatches")
    assert n_spread == 0 and n_place == 6
    assert n_step >= 4 * 800
