"""Parity of the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs.

Bars: neighbour pair SET bit-exact against the same-precision oracle; fp64 forces |ΔF| <= 1e-7 kJ/mol/nm
and |ΔE| <= 1e-5 kJ/mol-scale relative (the reference's own bars, test/protein.jl:267,274;
test/gpu_consistency.jl:44 rtol 1e-8); fp32 forces within 4e-5·Σ_j‖f_ij‖ per atom (+ the force jump of
pairs within 2e-6 of a hard cutoff) and a relative RMS force error no worse than 1.5x that of the reference's own
arithmetic evaluated in fp32 (tests/systems.py:fp32_reference_rms), fp32 energies within 2e-5 relative.
"""
import math

import numpy as np
import pytest

from tests import systems as S

pytestmark = pytest.mark.gpu


def nl_keys(i, j, sp):
    lo, hi, s = S.sorted_pairs(i, j, sp)
    return lo, hi, s


def assert_same_neighbors(m, case, dtype):
    o = case.oracle(dtype)
    oi, oj, osp = o.neighbors("cell", nthreads=4)
    sys_ = case.system(m, dtype)
    nl = m.find_neighbors(sys_)
    a, b = nl_keys(oi, oj, osp), nl_keys(nl.i, nl.j, nl.special)
    assert len(a[0]) == len(b[0]), f"{case.name}: {len(b[0])} pairs, oracle {len(a[0])}"
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    return sys_, (oi, oj, osp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("maker", ["lj16", "lj8_small_box", "charged12", "lj20"])
def test_neighbor_set_bit_exact(pkg, maker, dtype):
    case = {"lj16": lambda: S.lj_fluid(16, dtype=dtype), "lj8_small_box": lambda: S.lj_fluid(8, dtype=dtype),
            "charged12": lambda: S.charged_fluid(12, dict(kind="rf", rc=1.0), dtype=dtype),
            "lj20": lambda: S.lj_fluid(20, seed=9, jitter=0.05, dtype=dtype)}[maker]()
    sys_, _ = assert_same_neighbors(pkg, case, dtype)
    st = sys_.stats()
    assert st["n_pairs_full"] % 2 == 0
    if maker == "lj8_small_box":
        assert st["minimg_mode"] == 1   # box 2.9 nm < 2·(block half-extent + r_list): in-loop exact minimum image


def test_neighbor_three_atom_toy(pkg):
    # test/basic.jl:494-518
    case = S.Case([[1, 1, 1], [2, 2, 2], [5, 5, 5]], 10.0, lj=dict(cutoff=("distance", 1.0)), r_list=2.0,
                  sigma=np.full(3, 0.3), eps=np.full(3, 0.2))
    nl = pkg.find_neighbors(case.system(pkg, np.float64))
    assert nl.list == [(0, 1, False)]


COULS = {
    "plain_none": dict(kind="plain", cutoff=("none",)),
    "plain_dist": dict(kind="plain", cutoff=("distance", 1.0), weight_special=0.8333333333333334),
    "plain_shifted_force": dict(kind="plain", cutoff=("shifted_force", 1.0)),
    "rf": dict(kind="rf", rc=1.0, eps_rf=78.3, weight_special=0.8333333333333334),
    "rf_inf": dict(kind="rf", rc=1.0, eps_rf=math.inf),
    "ewald": dict(kind="ewald", rc=1.0, weight_special=0.8333333333333334),
    "ewald_exact_erfc": dict(kind="ewald", rc=1.0, approx=False),
}


@pytest.mark.parametrize("coul", sorted(COULS))
def test_forces_and_energy_fp64(pkg, coul):
    case = S.charged_fluid(12, COULS[coul], dtype=np.float64)
    o = case.oracle(np.float64)
    nl = o.neighbors("cell")
    f_ref, e_ref = o.forces(nl), o.potential_energy(nl)
    s = case.system(pkg, np.float64)
    f = pkg.forces(s)
    fmax = np.abs(f_ref).max()
    assert np.abs(f - f_ref).max() <= 1e-9 * fmax + 1e-7
    e = pkg.potential_energy(s)
    assert e == pytest.approx(e_ref, rel=1e-10, abs=1e-6)


@pytest.mark.parametrize("coul", ["rf", "ewald", "plain_dist"])
def test_forces_and_energy_fp32(pkg, coul):
    case = S.charged_fluid(14, COULS[coul], dtype=np.float32)
    tol, o, nl = S.fp32_force_tolerance(case)
    f_ref = o.forces(nl)
    s = case.system(pkg, np.float32)
    f = pkg.forces(s).astype(np.float64)
    err = np.linalg.norm(f - f_ref, axis=1)
    S.fp32_check(err, tol)
    assert S.rel_rms(err, f_ref) <= max(1.5 * S.fp32_reference_rms(case, f_ref), 5e-6)
    e_ref = o.potential_energy(nl)
    e = pkg.potential_energy(s)
    # Σ|e_ij| scale: use the fp64 oracle energy of the absolute values via a generous proxy
    assert e == pytest.approx(e_ref, rel=2e-5, abs=2e-6 * case.n * 500)


@pytest.mark.parametrize("kind", ["none", "distance", "shifted_potential", "shifted_force", "cubic_spline", "polynomial"])
def test_all_cutoffs_lj_fp64(pkg, kind):
    # the six strategies of cutoffs.jl on a 1000-atom fluid (energy-conservation systems use them: test/energy_conservation.jl:21-26)
    base = S.lj_fluid(10, dtype=np.float64)
    cut = (kind,) if kind == "none" else ((kind, 1.0, 0.8) if kind in ("cubic_spline", "polynomial") else (kind, 1.0))
    case = S.Case(base.coords, base.box, lj=dict(cutoff=cut), r_list=1.2 if kind != "none" else 1.7, sigma=base.sigma, eps=base.eps, mass=base.mass)
    o = case.oracle(np.float64)
    nl = o.neighbors("cell")
    s = case.system(pkg, np.float64)
    f_ref = o.forces(nl)
    assert np.abs(pkg.forces(s) - f_ref).max() <= 1e-9 * np.abs(f_ref).max() + 1e-8
    assert pkg.potential_energy(s) == pytest.approx(o.potential_energy(nl), rel=1e-10, abs=1e-8)


def test_no_neighbor_list_path(pkg):
    # README example shape (README.md:72-95) and test/gpu_consistency.jl:407-449: NoCutoff, no neighbour finder
    rng = np.random.default_rng(1)
    n = 100
    g = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * 0.4 + 0.1
    x = g + rng.uniform(-0.03, 0.03, (n, 3))
    case = S.Case(x, 2.0, lj=dict(cutoff=("none",)), coul=dict(kind="plain", cutoff=("none",)), sigma=np.full(n, 0.3),
                  eps=np.full(n, 0.2), mass=np.full(n, 10.0), charge=rng.normal(size=n) * 0.1)
    o = case.oracle(np.float64)
    f_ref = o.forces(None)
    s = case.system(pkg, np.float64)
    assert np.abs(pkg.forces(s) - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
    assert pkg.potential_energy(s) == pytest.approx(o.potential_energy(None), rel=1e-10)
    assert pkg.find_neighbors(s) is None


def test_gpu_consistency_diagonal_33_atoms(pkg):
    # test/gpu_consistency.jl:3-50: 33 atoms on a diagonal (0.5·i), box 20, LJ σ=1? rc 5 — partial tile
    n = 33
    x = np.array([[0.5 * (i + 1)] * 3 for i in range(n)])
    case = S.Case(x, 20.0, lj=dict(cutoff=("distance", 5.0)), r_list=5.0, sigma=np.full(n, 0.3), eps=np.full(n, 0.2), mass=np.full(n, 10.0))
    o = case.oracle(np.float64)
    nl = o.neighbors("brute")
    s = case.system(pkg, np.float64)
    np.testing.assert_allclose(pkg.forces(s), o.forces(nl), rtol=1e-8, atol=1e-10)
    assert pkg.potential_energy(s) == pytest.approx(o.potential_energy(nl), rel=1e-8, abs=1e-10)


def test_gpu_consistency_lattice_100_atoms(pkg):
    # test/gpu_consistency.jl:52-114: 100-atom lattice spacing 1.5, σ = 1, rc 4 (lattice distances hit exact ties)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(float)
    x = g * 1.5 + 0.75
    n = len(x)
    case = S.Case(x, 9.0, lj=dict(cutoff=("distance", 4.0)), r_list=4.0, sigma=np.full(n, 1.0), eps=np.full(n, 0.2), mass=np.full(n, 10.0))
    for dtype in (np.float64, np.float32):
        o = case.oracle(dtype)
        oi, oj, osp = o.neighbors("brute")
        s = case.system(pkg, dtype)
        nl = pkg.find_neighbors(s)
        a, b = nl_keys(oi, oj, osp), nl_keys(nl.i, nl.j, nl.special)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    o = case.oracle(np.float64)
    nl = o.neighbors("brute")
    s = case.system(pkg, np.float64)
    np.testing.assert_allclose(pkg.forces(s), o.forces(nl), rtol=1e-8, atol=1e-9)


def test_exclusions_and_special_pairs(pkg):
    # test/gpu_consistency.jl:339-405: 10 atoms, excluded (1,2),(2,3), special (1,3) [1-based]
    rng = np.random.default_rng(4)
    x = rng.random((10, 3)) * 1.2 + 0.4
    case = S.Case(x, 6.0, lj=dict(cutoff=("distance", 2.0), weight_special=0.5), coul=dict(kind="plain", cutoff=("distance", 2.0), weight_special=0.8),
                  r_list=2.5, sigma=np.full(10, 0.25), eps=np.full(10, 0.3), charge=rng.normal(size=10) * 0.4,
                  excluded=[[0, 1], [1, 2]], special=[[0, 2]])
    o = case.oracle(np.float64)
    oi, oj, osp = o.neighbors("brute")
    s = case.system(pkg, np.float64)
    nl = pkg.find_neighbors(s)
    keys = set(zip(nl.i.tolist(), nl.j.tolist()))
    assert (0, 1) not in keys and (1, 2) not in keys and (0, 2) in keys
    assert dict(zip(zip(nl.i.tolist(), nl.j.tolist()), nl.special.tolist()))[(0, 2)] == 1
    np.testing.assert_allclose(pkg.forces(s), o.forces((oi, oj, osp)), rtol=1e-8, atol=1e-9)
    # cache invalidation after changing the exceptions (test/gpu_consistency.jl:494-527)
    case2 = S.Case(x, 6.0, lj=case.lj, coul=case.coul, r_list=2.5, sigma=case.sigma, eps=case.eps, charge=case.charge,
                   excluded=[[0, 1], [1, 2], [3, 4]], special=[[0, 2]])
    s.neighbor_finder = pkg.GPUNeighborFinder(dist_cutoff=2.5, excluded_pairs=case2.excluded, special_pairs=case2.special)
    s._push_atoms()
    o2 = case2.oracle(np.float64)
    np.testing.assert_allclose(pkg.forces(s), o2.forces(o2.neighbors("brute")), rtol=1e-8, atol=1e-9)


def test_buffer_reuse_after_moving_coords(pkg):
    # test/gpu_consistency.jl:451-492
    case = S.lj_fluid(12, dtype=np.float64)
    s = case.system(pkg, np.float64)
    pkg.forces(s)
    rng = np.random.default_rng(8)
    x2 = case.coords + rng.normal(size=case.coords.shape) * 0.05
    x2 = x2 - np.floor(x2 / case.box) * case.box
    s.coords[:] = x2
    o = case.oracle(np.float64, coords=x2)
    f_ref = o.forces(o.neighbors("cell"))
    assert np.abs(pkg.forces(s, step_n=1) - f_ref).max() <= 1e-9 * np.abs(f_ref).max() + 1e-8


def test_remove_cm_motion_and_kinetic_energy(pkg):
    # test/gpu_consistency.jl:116-157
    case = S.charged_fluid(10, dict(kind="rf", rc=1.0), dtype=np.float64)
    rng = np.random.default_rng(2)
    v = rng.normal(size=(case.n, 3)) + np.array([0.3, -0.2, 0.1])
    s = case.system(pkg, np.float64, velocities=v)
    o = case.oracle(np.float64, velocities=v)
    assert pkg.kinetic_energy(s) == pytest.approx(o.kinetic_energy(), rel=1e-12)
    pkg.remove_CM_motion(s)
    o.remove_cm()
    np.testing.assert_allclose(s.velocities, o.vel, rtol=0, atol=1e-12)
    assert np.abs((s.velocities * case.mass[:, None]).sum(axis=0)).max() < 1e-9


def test_sorted_order_is_a_permutation(pkg):
    # reorder / reverse-reorder round trip (test/gpu_optimizations.jl:220-250)
    import ctypes as C
    case = S.lj_fluid(12, dtype=np.float32)
    s = case.system(pkg, np.float32)
    f1 = pkg.forces(s)
    perm = np.empty(case.n, np.int32)
    s._check(pkg.lib().mhip_export_order(s.engine(), perm.ctypes.data_as(C.c_void_p), case.n))
    assert np.array_equal(np.sort(perm), np.arange(case.n))
    assert not np.array_equal(perm, np.arange(case.n))   # the Hilbert sort really reordered the atoms
    s.pull_state()
    np.testing.assert_array_equal(s.coords, case.coords.astype(np.float32))   # state round-trips bit-exactly
    assert np.array_equal(pkg.forces(s), f1)   # and forces are bit-reproducible (no atomics on the pair path)


def test_velocity_verlet_fp64_matches_oracle(pkg):
    case = S.charged_fluid(10, dict(kind="rf", rc=1.0), dtype=np.float64, with_exceptions=True, stable=True)
    o = case.oracle(np.float64)
    o.vv_run(40, 0.0005, remove_cm_every=1)
    s = case.system(pkg, np.float64)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 40)
    assert np.abs(s.coords - o.coords).max() < 1e-9      # reference bar 1e-10 nm vs OpenMM over 100 steps (protein.jl:289)
    assert np.abs(s.velocities - o.vel).max() < 1e-7


def test_velocity_verlet_fp32_lj_tracks_fp64_oracle(pkg):
    # test/simulation.jl:625: mean |Δx| < 5e-4 nm after 100 steps at fp32
    case = S.lj_fluid(12, dtype=np.float32)
    o = case.oracle(np.float64)
    o.vv_run(100, 0.002, remove_cm_every=1)
    s = case.system(pkg, np.float32)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002), 100)
    d = s.coords.astype(np.float64) - o.coords
    d -= np.round(d / case.box) * case.box
    assert np.abs(d).mean() < 5e-4
    assert np.abs((s.velocities.astype(np.float64) * case.mass[:, None]).sum(axis=0)).max() < 1e-2


def test_chunked_continuation(pkg):
    # test/simulation.jl:16-57: 10 steps == 3 + 3 + 4 with init_step 3, 6.  The reference compares with exact
    # == on the CPU (its pair order is history-independent); here each chunk start re-sorts the atoms, which
    # permutes fp32 summation orders, so the chunked run agrees to rounding, while step numbering / rebuild
    # cadence are exact and a chunk boundary on a rebuild step changes nothing but that.
    case = S.lj_fluid(10, dtype=np.float32)
    a = case.system(pkg, np.float32)
    pkg.simulate(a, pkg.VelocityVerlet(dt=0.002), 10)
    b = case.system(pkg, np.float32)
    pkg.simulate(b, pkg.VelocityVerlet(dt=0.002), 3)
    pkg.simulate(b, pkg.VelocityVerlet(dt=0.002), 3, init_step=3)
    pkg.simulate(b, pkg.VelocityVerlet(dt=0.002), 4, init_step=6)
    d = a.coords.astype(np.float64) - b.coords
    d -= np.round(d / case.box) * case.box
    assert np.abs(d).max() < 5e-6 and np.abs(a.velocities - b.velocities).max() < 5e-5
    # the same chunking twice is bit-identical (no atomics, history-independent sort)
    c = case.system(pkg, np.float32)
    pkg.simulate(c, pkg.VelocityVerlet(dt=0.002), 3)
    pkg.simulate(c, pkg.VelocityVerlet(dt=0.002), 3, init_step=3)
    pkg.simulate(c, pkg.VelocityVerlet(dt=0.002), 4, init_step=6)
    assert np.array_equal(b.coords, c.coords) and np.array_equal(b.velocities, c.velocities)
    # fp64: the chunked run reproduces the continuous one to 1e-12
    a = case.system(pkg, np.float64); pkg.simulate(a, pkg.VelocityVerlet(dt=0.002), 10)
    b = case.system(pkg, np.float64)
    for first, n in ((0, 3), (3, 3), (6, 4)):
        pkg.simulate(b, pkg.VelocityVerlet(dt=0.002), n, init_step=first)
    assert np.abs(a.coords - b.coords).max() < 1e-12 and np.abs(a.velocities - b.velocities).max() < 1e-11


def test_nve_energy_conservation_short(pkg):
    # test/energy_conservation.jl:13-77 scaled down: σ = 0.05 LJ gas, T = 1 K, dt = 1 fs, no CM removal
    rng = np.random.default_rng(0)
    n, box = 2000, 5.0
    g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * (box / 13) + 0.1
    x = g + rng.uniform(-0.05, 0.05, (n, 3))
    v = rng.normal(size=(n, 3)) * math.sqrt(8.314462618e-3 * 1.0 / 40.0)
    case = S.Case(x, box, lj=dict(cutoff=("shifted_force", 2.0)), r_list=2.3, velocities=v, sigma=np.full(n, 0.05), eps=np.full(n, 0.2), mass=np.full(n, 40.0))
    s = case.system(pkg, np.float64)
    e0 = pkg.total_energy(s)
    es = []
    for k in range(5):
        pkg.simulate(s, pkg.VelocityVerlet(dt=0.001, remove_CM_motion=0), 400, init_step=400 * k)
        es.append(pkg.total_energy(s))
    assert max(abs(e - e0) for e in es) < 5e-4


def test_bonded_terms_match_oracle(pkg):
    # a synthetic 60-bead chain with bonds, angles, torsions (2 Fourier terms each) and Ewald exclusions (tests/bonded_ref.py: bead_chain).  Per atom against
    # S_i = Σ over its terms of the norm of the term's force on it — 1e-9·S_i in fp64, twice the fp32 oracle's own loss in fp32 (test_bonded_host.YARD32) — AND
    # the former bar against the largest force component, so that no atom's bar got looser: the chain's largest force is a bond force of 1e4 kJ/mol/nm, three
    # hundred times its torsion forces.
    from tests import bonded_ref as R
    from tests.test_bonded_host import YARD32
    case = R.bead_chain()
    scale = R.per_atom_scale(case)
    assert np.all(scale > 0)
    for dtype, rtol, bar in ((np.float64, 1e-9, 1e-9), (np.float32, 3e-4, 2.0 * YARD32["bead_all"][0])):
        o = case.oracle(np.float64)
        f_ref = o.forces(None, pairwise=False, specific=True)
        e_ref = o.potential_energy(None, pairwise=False, specific=True)
        s = case.system(pkg, dtype)
        f = pkg.forces(s, pairwise=False)
        assert np.abs(f - f_ref).max() <= rtol * np.abs(f_ref).max()
        ratio = np.linalg.norm(f.astype(np.float64) - f_ref, axis=1) / scale
        print(f"[bonded] bead chain {np.dtype(dtype).name}: worst ‖Δf_i‖/S_i {ratio.max():.3e} (bar {bar:.3e})")
        assert ratio.max() <= bar, (ratio.max(), int(ratio.argmax()))
        assert pkg.potential_energy(s, pairwise=False) == pytest.approx(e_ref, rel=max(rtol, 1e-9))


def test_full_size_256k_lj_against_oracle(pkg):
    """BASELINE.json configs[1]: 262 144-atom LJ fluid, fp32 — direct comparison with the fp64 oracle plus the
    size-independent properties (Newton's third law ΣF = 0, full list symmetric = 2 × half list)."""
    case = S.lj_fluid(64, dtype=np.float32)
    tol, o, nl = S.fp32_force_tolerance(case)
    f_ref = o.forces(nl, nthreads=8)
    s = case.system(pkg, np.float32)
    f = pkg.forces(s).astype(np.float64)
    err = np.linalg.norm(f - f_ref, axis=1)
    S.fp32_check(err, tol)
    assert S.rel_rms(err, f_ref) <= max(1.5 * S.fp32_reference_rms(case, f_ref), 5e-6)
    # Newton's third law: both directions of a pair are evaluated independently in fp32, so ΣF vanishes to rounding
    assert np.abs(f.sum(axis=0)).max() < 1e-6 * o.pair_force_scale.sum()
    st = s.stats()
    o32 = case.oracle(np.float32)
    oi, oj, _ = o32.neighbors("cell", nthreads=8)
    assert st["n_pairs_full"] == 2 * len(oi)
    assert st["minimg_mode"] == 0
    # the pair SET, not only its size: 20 M pairs bit-identical to the fp32 reference search
    keys, n_special = S.export_keys(pkg, s)
    assert n_special == 0 and np.array_equal(keys, S.pair_keys(oi, oj))
    # the pass above walked the OUTER list and pruned it on the way (the PRUNE variant of the kernel); the next one walks the inner
    # list with the packed loop: the same partners inside the cutoff in the same order, each rounded together with another list
    # neighbour (two partners share one reciprocal) — same bar, and the two passes agree far inside it
    f2 = pkg.forces(s).astype(np.float64)
    assert s.stats()["n_filter_passes"] == st["n_filter_passes"]
    err2 = np.linalg.norm(f2 - f_ref, axis=1)
    assert np.all(err2 <= tol) and np.all(np.linalg.norm(f2 - f, axis=1) <= 0.25 * tol)
    e_ref = o.potential_energy(nl)
    assert pkg.potential_energy(s) == pytest.approx(e_ref, rel=2e-5)
    # … and after dynamics: 40 steps (prunes of the inner list on the way), then forces through the lists in use against a fresh
    # reference evaluation of the coordinates reached
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002), 40)
    assert s.stats()["n_filter_passes"] > st["n_filter_passes"]
    tol3, o3, nl3 = S.fp32_force_tolerance(case, coords=s.coords.astype(np.float64))
    f3 = pkg.forces(s, step_n=40).astype(np.float64)
    err3 = np.linalg.norm(f3 - o3.forces(nl3, nthreads=8), axis=1)
    S.fp32_check(err3, tol3, "fp32 forces after a prune")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dual_pair_list_stays_bit_exact_during_a_run(pkg, dtype):
    """The engine searches with r_list + 0.1 nm every 5th rebuild interval and FILTERS that outer list to exactly r_list at
    every rebuild step.  After 30 steps (filter passes at 10, 20, 30) the list it is using must equal a fresh reference
    search on the coordinates it holds — same pair set, same special flags."""
    import ctypes as C
    case = S.charged_fluid(12, dict(kind="rf", rc=1.0), dtype=dtype, stable=True)
    s = case.system(pkg, dtype)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.001), 30)
    L = pkg.lib()
    n = C.c_int64(0)
    s._check(L.mhip_export_neighbors(s.engine(), None, None, None, 0, C.byref(n)))
    i = np.empty(n.value, np.int32); j = np.empty(n.value, np.int32); sp = np.empty(n.value, np.uint8)
    s._check(L.mhip_export_neighbors(s.engine(), s._ptr(i), s._ptr(j), s._ptr(sp), n.value, C.byref(n)))
    st = s.stats()
    o = case.oracle(dtype, coords=s.coords.astype(np.float64))
    oi, oj, osp = o.neighbors("cell", nthreads=4)
    a, b = nl_keys(oi, oj, osp), nl_keys(i, j, sp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert st["n_rebuilds"] >= 4


@pytest.mark.parametrize("kind,dtype", [("lj", np.float64), ("lj", np.float32), ("rf", np.float64), ("ewald", np.float32)])
def test_pairwise_virial_vs_oracle(pkg, kind, dtype):
    """mhip_forces(virial9): Σ dr ⊗ f over the pair list (≙ needs_vir, force.jl:848-852, 877-880), against the oracle, whose trace
    satisfies tr W = −dE/dλ under uniform scaling (tests/test_oracle_golden.py)"""
    if kind == "lj":
        case = S.lj_fluid(12, dtype=dtype)
    else:
        case = S.charged_fluid(10, dict(kind=kind, rc=1.0, weight_special=0.8333333333333334), dtype=dtype, stable=True)
    o = case.oracle(np.float64)
    w_ref = o.virial(o.neighbors("cell"))
    s = case.system(pkg, dtype)
    w = pkg.virial(s)
    scale = np.abs(w_ref).max()
    assert np.abs(w - w_ref).max() < (1e-10 if dtype == np.float64 else 2e-4) * scale
    assert np.abs(w - w.T).max() == 0.0
    assert pkg.scalar_virial(s) == pytest.approx(np.trace(w), rel=1e-12)
    f = pkg.forces(s)                                   # the virial call left the engine's forces untouched
    assert np.isfinite(f).all()


@pytest.mark.parametrize("n_steps,cm_every,first", [(1, 1, 5), (2, 1, 5), (7, 3, 4), (12, 1, 0), (6, 0, 2)])
def test_fused_velocity_verlet_with_net_momentum_matches_oracle(pkg, n_steps, cm_every, first):
    """vv_run's one-launch-per-step form (k_vv_mid) applies remove_CM_motion! one launch late, to the velocity AND to the position that
    was drifted with it.  A system with a large net momentum entered at init_step > 0 (no up-front removal, simulators.jl:563) makes
    that shift visible: v_cm·dt ≈ 1e-3 nm.  Also the run lengths around the first / last step special cases and a 3-step CM cadence."""
    case = S.lj_fluid(8, dtype=np.float64)
    case.velocities = case.velocities + np.array([0.6, -0.4, 0.25])
    o = case.oracle(np.float64)
    o.vv_run(n_steps, 0.002, first_step=first, remove_cm_every=cm_every)
    s = case.system(pkg, np.float64)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002, remove_CM_motion=cm_every), n_steps, init_step=first)
    d = s.coords - o.coords
    d -= np.round(d / case.box) * case.box
    assert np.abs(d).max() < 1e-10 and np.abs(s.velocities - o.vel).max() < 1e-9
    f_ref = o.forces(o.neighbors("cell"))
    assert np.abs(pkg.forces(s) - f_ref).max() < 1e-7 * np.abs(f_ref).max()


@pytest.mark.parametrize("kind,n_side", [("lj", 40), ("lj", 48), ("charged", 36), ("charged", 48), ("charged", 14)])
def test_single_pair_list_with_128_and_256_atom_blocks(pkg, kind, n_side, monkeypatch):
    """The single (non-dual) pair list — what a context falls back to when the dual list does not pay or does not fit, and what a sub-domain without a
    ghost margin uses — at the sizes where the blocks hold 128 (40 000+ atoms) and 256 atoms (100 000+).  Round 5 found the search with exact band
    decisions AND exception lookups compiled in leaving every i-wave but the first of such blocks with an empty list (half / three quarters of the
    pairs gone; tools/micro/xl_waves.py), on exception-free systems too, because they were routed through the same instantiation; nothing in the
    suite built a single list beyond 64-atom blocks.  Pair SET against the oracle's of the same precision, forces against the fp64 oracle."""
    monkeypatch.setenv("MOLLYHIP_OUTER_MARGIN_PM", "0")
    if kind == "lj":
        case = S.lj_fluid(n_side, dtype=np.float32)
    else:
        case = S.charged_fluid(n_side, dict(kind="rf", rc=1.0, weight_special=0.8333333333333334), dtype=np.float32, stable=True)
    s = case.system(pkg, np.float32)
    tol, o, nl = S.fp32_force_tolerance(case)
    f_ref = o.forces(nl, nthreads=16)
    f = pkg.forces(s).astype(np.float64)
    st = s.stats()
    # the charged cases run the walk with exact band decisions AND exception lookups compiled in (k_build<T, true, false, true>) at 64 x 16 (n_side 14), 128 x 4 (36)
    # and 256 x 2 (48): the variant whose defect round 6 bisected to private arrays in scratch (engine.hip rebuild_impl) and that was detoured beyond 64-atom blocks until then
    assert st["block_atoms"] >= 128 or n_side == 14, st["block_atoms"]
    assert n_side != 14 or st["block_atoms"] == 64
    assert (kind, n_side) != ("charged", 48) or st["block_atoms"] == 256
    err = np.linalg.norm(f - f_ref, axis=1)
    S.fp32_check(err, tol)
    keys, n_special = S.export_keys(pkg, s)
    oi, oj, osp = case.oracle(np.float32).neighbors("cell", nthreads=16)
    assert np.array_equal(keys, S.pair_keys(oi, oj)) and n_special == int(np.asarray(osp).sum())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_per_atom_lambda_zero_switches_the_lennard_jones_pair_off(pkg, dtype):
    """Atom.λ (types.jl:466-475) enters the unsoftened interactions through the LJZeroShortcut alone: a pair with λ = 0 on either side has no
    Lennard-Jones force or energy (mixing.jl:7-11), its Coulomb part is untouched (coulomb.jl:81 reads the charge only), and it STAYS in the
    neighbour list (neighbors.jl:409-411 knows nothing of λ).  mhip_set_atoms(lambda) against the oracle's restatement of the shortcut: forces,
    energy and the pair set, with every seventh atom at λ = 0, a few at λ = 0.5 (no effect without soft core) and the rest at 1."""
    base = S.charged_fluid(12, dict(kind="rf", rc=1.0, weight_special=0.8333333333333334), dtype=dtype, stable=True)
    lam = np.ones(base.n)
    lam[::7] = 0.0
    lam[3::11] = 0.5
    case = S.Case(base.coords, base.box, lj=base.lj, coul=base.coul, r_list=base.r_list, rebuild_every=base.rebuild_every, velocities=base.velocities,
                  charge=base.charge, sigma=base.sigma, eps=base.eps, mass=base.mass, excluded=base.excluded, special=base.special, lam=lam)
    s = case.system(pkg, dtype)
    off = lam == 0
    assert s.λ is not None and (s.λ == 0).sum() == off.sum()
    f = pkg.forces(s).astype(np.float64)
    if dtype == np.float64:
        o = case.oracle(np.float64)
        nl = o.neighbors("cell")
        f_ref = o.forces(nl)
        assert np.abs(f - f_ref).max() <= 1e-9 * np.abs(f_ref).max() + 1e-7
        assert pkg.potential_energy(s) == pytest.approx(o.potential_energy(nl), rel=1e-10, abs=1e-6)
    else:
        tol, o, nl = S.fp32_force_tolerance(case)
        f_ref = o.forces(nl)
        S.fp32_check(np.linalg.norm(f - f_ref, axis=1), tol, "fp32 forces with per-atom λ")
    # the shortcut really bites: the same system with every λ = 1 has other forces on the λ = 0 atoms (and on their neighbours) …
    f_all = base.oracle(np.float64).forces(base.oracle(np.float64).neighbors("cell"))
    assert np.linalg.norm(f_all - f_ref, axis=1)[off].max() > 1e-2 * np.linalg.norm(f_all, axis=1).mean()
    # … and equals the system whose λ = 0 atoms have ϵ = 0 instead (the engine folds λ = 0 in as σ = ϵ = 0: DESIGN §3)
    eps0 = np.where(lam == 0, 0.0, np.broadcast_to(np.asarray(base.eps, dtype=np.float64), (base.n,)))
    twin = S.Case(base.coords, base.box, lj=base.lj, coul=base.coul, r_list=base.r_list, rebuild_every=base.rebuild_every, charge=base.charge, sigma=base.sigma,
                  eps=eps0, mass=base.mass, excluded=base.excluded, special=base.special).oracle(np.float64)
    assert np.abs(twin.forces(twin.neighbors("cell")) - f_ref).max() <= 1e-12 * np.abs(f_ref).max()
    # λ does not touch the neighbour list
    keys, n_special = S.export_keys(pkg, s)
    oi, oj, osp = case.oracle(dtype).neighbors("cell")
    assert np.array_equal(keys, S.pair_keys(oi, oj)) and n_special == int(np.asarray(osp).sum())
    # a one-type LJ fluid with some λ = 0 atoms must leave the uniform fast path (k_uniform_check) and still be right
    lj = S.lj_fluid(12, dtype=dtype)
    lam2 = np.ones(lj.n); lam2[5::9] = 0.0
    case2 = S.Case(lj.coords, lj.box, lj=lj.lj, r_list=lj.r_list, rebuild_every=lj.rebuild_every, velocities=lj.velocities, sigma=lj.sigma, eps=lj.eps, mass=lj.mass, lam=lam2)
    o2 = case2.oracle(np.float64)
    f2_ref = o2.forces(o2.neighbors("cell"))
    f2 = pkg.forces(case2.system(pkg, dtype)).astype(np.float64)
    assert np.abs(f2[lam2 == 0]).max() == 0.0 and np.abs(f2_ref[lam2 == 0]).max() == 0.0
    assert np.abs(f2 - f2_ref).max() <= (1e-9 if dtype == np.float64 else 2e-4) * np.abs(f2_ref).max()
