"""The specific interactions on the device (csrc/bonded.h: k_bonded + k_bonded_collect, the energy and virial kernels; step_fused.h and forces_gs.hip: the same
terms as blocks of other launches) against the fp64 oracle, type by type, on small synthetic systems built to sit on the edges of the block-range arithmetic, of
the per-atom slot sums and of the geometry (tests/bonded_ref.py has the systems and the independent reference the per-atom scale S_i comes from).

Bars.  Every force comparison is per atom: ‖Δf_i‖ against S_i = Σ over the terms of atom i of the norm of that term's force on i.  fp64: 1e-9·S_i, energy 1e-11
relative, virial 1e-9 of its largest component.  fp32: twice what the oracle's own arithmetic in fp32 loses against itself in fp64 on systems of the same group
(tests/test_bonded_host.py: YARD32, measured on the CPU).  Near-degenerate geometry, fp64: twice the disagreement of the fp64 oracle with the longdouble reference
(ORACLE_VS_REF).  What is stated as exact is compared with ==."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import bonded_ref as R
from tests import systems as S  # noqa: F401  (Case.oracle)
from tests.test_bonded_host import EPS32, EPS64, ORACLE_VS_REF, RUN_STEPS, YARD32, YARD32_RUN, zero_charge_only

pytestmark = pytest.mark.gpu

FP64_BARS = (1e-9, 1e-11, 1e-9)
DTYPES = [np.float64, np.float32]


PLANAR = ("torsion_planar", "torsion_near_pi", "near_collinear_1e-3", "near_collinear_1e-5")


def bars(group, dtype, near=False):
    """(forces, energy, virial).  A measured figure below one unit of roundoff only says that the host's arithmetic happened to be exact on those inputs: the bars
    stop at that unit.  The virial of the planar torsions and of the near-collinear angles all but vanishes and is measured against Σ‖r‖‖f‖ (bonded_ref.group_wscale); an error of δ·S_i in the
    forces moves it by at most δ·Σ‖r‖‖f‖, so it takes the force bar."""
    if dtype == np.float32:
        b = [2.0 * max(y, EPS32) for y in YARD32[group]]
    else:
        b = [2.0 * max(y, EPS64) for y in ORACLE_VS_REF[group]] if near else list(FP64_BARS)
    if group in PLANAR:
        b[2] = b[0]
    return tuple(b)


def device_all(pkg, s):
    return (pkg.forces(s, pairwise=False).astype(np.float64), pkg.potential_energy(s, pairwise=False), pkg.virial(s, pairwise=False, general=False))


_ref_cache = {}


def reference(group, case):
    """fp64 oracle (forces, energy, virial) and the per-atom scale of a case — computed once per system, shared by its fp64 and fp32 runs, never modified"""
    key = (group, case.name)
    if key not in _ref_cache:
        f, e, w = R.oracle_all(case, np.float64)
        sc = R.group_scale(group, case)
        for a in (f, w, sc): a.setflags(write=False)
        _ref_cache[key] = (f, e, w, sc, R.group_wscale(group, case))
    return _ref_cache[key]


def check(pkg, group, case, dtype, near=False, s=None):
    f_ref, e_ref, w_ref, scale, wscale = reference(group, case)
    s = s if s is not None else case.system(pkg, dtype)
    f, e, w = device_all(pkg, s)
    rf, re, rw, n_cmp = R.compare(f, e, w, f_ref, e_ref, w_ref, scale, wscale)
    bf, be, bw = bars(group, dtype, near)
    print(f"[bonded] {group} {case.name} {np.dtype(dtype).name}: force {rf:.3e} (bar {bf:.3e})  energy {re:.3e} (bar {be:.3e})  virial {rw:.3e} (bar {bw:.3e})  atoms compared {n_cmp}")
    assert np.isfinite(f).all() and math.isfinite(e) and np.isfinite(w).all()
    # coverage: the atoms compared are the atoms the TOPOLOGY puts into a term (less those whose only terms are exclusions with a zero charge product, which
    # have no force by definition) — counted from the term lists, not from the scale — and every other atom must have exactly no force
    slots = R.slot_counts(case)
    expected = (slots > 0) & ~zero_charge_only(case, slots)
    assert np.array_equal(scale > 0, expected) and n_cmp == int(expected.sum())
    assert np.all(f[~expected] == 0.0), "an atom without any term force got a force"
    assert rf <= bf, f"forces: worst ‖Δf_i‖/S_i {rf:.3e} > {bf:.3e}"
    assert re <= be, f"energy: {re:.3e} > {be:.3e} ({e} vs {e_ref})"
    assert rw <= bw, f"virial: {rw:.3e} > {bw:.3e}"
    return s, f


# ---- a. term counts at block edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", R.COUNTS)
@pytest.mark.parametrize("ty", R.TYPES)
def test_one_type_alone_at_block_edges(pkg, ty, n, dtype):
    """n terms of one type, the other three absent: one term, one short of a 64-lane block, a full block, one over, two blocks and one"""
    case = R.chains(seed=0, **{R.KW[ty]: n})
    assert R.n_terms(case) == {**dict.fromkeys(R.TYPES, 0), ty: n} and case.n % 32 != 0
    check(pkg, f"a_{ty}", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1])
def test_mixed_types_at_block_edges(pkg, which, dtype):
    """0: every type present with n ≡ 1 (mod 64); 1: bonds and torsions only — an empty block range in the middle (angles) and at the end (exclusions)"""
    case = R.mixed_cases(0)[which]
    nt = R.n_terms(case)
    assert all(v % 64 == 1 for v in nt.values()) if which == 0 else (nt["angles"] == 0 and nt["excl"] == 0 and nt["bonds"] and nt["torsions"])
    check(pkg, "a_mixed", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_types_in_a_triclinic_cell(pkg, dtype):
    """65 terms of every type on chains that cross the faces of a sheared cell: angles, torsions and exclusions take the cell's minimum image too, and the virial
    sink's origin (the term's first atom, where the oracle takes the second) does not show"""
    check(pkg, "tri", R.regular_groups(0)["tri"][0], dtype)


# ---- b. no type hides behind another ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", R.TYPES)
def test_bead_chain_each_type_alone_fp32(pkg, ty):
    """the 60-bead chain of test_gpu_parity.py with one type at a time: a torsion force is no longer measured against a bond force"""
    check(pkg, f"bead_{ty}", R.only(R.bead_chain(), ty), np.float32)


# ---- c. degenerate and near-degenerate geometry ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_collinear_angle_writes_zeros_over_a_stale_slot(pkg, dtype):
    """axis-aligned angles, straight and folded: ba × bc is exactly zero, the kernel's zero-writing path.  Evaluated on a context whose slots hold the forces of a
    bent geometry: exact zeros afterwards, energy k/2 (θ − θ0)² with θ = π and 0."""
    bent, flat = R.collinear_angles(bent=True), R.collinear_angles()
    s = bent.system(pkg, dtype)
    f0 = pkg.forces(s, pairwise=False)
    assert np.all(np.linalg.norm(f0, axis=1) > 100.0)                      # every slot holds a real force
    s.coords = flat.coords.astype(dtype)                                    # (forces() hands the state to the context)
    f = pkg.forces(s, pairwise=False)
    assert np.all(f == 0.0), f
    e_def = 384.0 / 2 * (math.pi - 1.75) ** 2 + 384.0 / 2 * 1.75 ** 2
    assert float(R.energy(flat)) == pytest.approx(e_def, rel=1e-14)
    rel = 1e-11 if dtype == np.float64 else 2.0 * YARD32["a_angles"][1]
    assert pkg.potential_energy(s, pairwise=False) == pytest.approx(e_def, rel=rel)
    assert np.all(pkg.virial(s, pairwise=False, general=False) == 0.0)
    # … and back: the zero slots are overwritten as well
    s.coords = bent.coords.astype(dtype)
    assert np.array_equal(pkg.forces(s, pairwise=False), f0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("group", ["near_collinear_1e-3", "near_collinear_1e-5", "torsion_near_pi", "face_bonds"])
def test_near_degenerate_geometry(pkg, group, dtype):
    """angles 1e-3 and 1e-5 rad off straight and off folded (the acos clamp); torsions 1e-4 rad on either side of ±π, periodicities 1–6, phases 0 and π; bonds through
    each face of the box with the atoms 1/64 nm from it"""
    case = R.degenerate_groups()[group][0]
    if group == "torsion_near_pi":
        phi = R.torsion_angles(case)
        assert np.all(np.abs(np.abs(phi) - (math.pi - 1e-4)) < 2e-6) and (phi > 0).any() and (phi < 0).any()
    check(pkg, group, case, dtype, near=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planar_torsions(pkg, dtype):
    """exactly planar cis and trans (atan2(±0, ±x): φ = 0 and π), periodicities 1–6, phases 0 and π: sin(nφ − phase) vanishes, so S_i does too (to the rounding of π),
    and the force is measured against what a torsion force CAN be there (bonded_ref.full_scale_torsions); energy k(1 ± 1)"""
    case = R.degenerate_groups()["torsion_planar"][0]
    phi = R.torsion_angles(case)
    assert set(np.round(phi, 12)) == {0.0, round(math.pi, 12)}
    assert np.all(R.group_scale("torsion_planar", case) > 0)
    check(pkg, "torsion_planar", case, dtype, near=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exclusion_pairs(pkg, dtype):
    """separations 1/64 nm and 1.0 nm, pairs with one charge zero (exactly no force); then coincident atoms: erf(αr) = 0, the zero-writing path and the limit energy —
    on the context that has just held real forces"""
    case = R.degenerate_groups()["excl_pairs"][0]
    s, f = check(pkg, "excl_pairs", case, dtype, near=True)
    q0 = np.nonzero(case.charge == 0.0)[0]
    assert len(q0) == 6 and np.all(f[q0] == 0.0) and np.all(f[q0 - 1] == 0.0)
    co = R.exclusion_pairs(coincident=True)
    for first in (True, False):            # a fresh context, then one whose slots hold the forces of separated pairs
        if first:
            sc = co.system(pkg, dtype)
        else:
            apart = co.coords.copy(); apart[1::2, 0] += R.U
            sc = co.system(pkg, dtype, coords=apart)
            assert np.all(np.linalg.norm(pkg.forces(sc, pairwise=False), axis=1) > 1.0)
            sc.coords = co.coords.astype(dtype)
        assert np.all(pkg.forces(sc, pairwise=False) == 0.0) and np.all(pkg.virial(sc, pairwise=False, general=False) == 0.0)
        alpha = co.inter_dict(dtype)["ewald_alpha"]
        e_def = 2 * (-2.0 * alpha * R.KE * (0.5 * -0.75) / math.sqrt(math.pi))
        assert pkg.potential_energy(sc, pairwise=False) == pytest.approx(e_def, rel=1e-11 if dtype == np.float64 else 4 * 2.0 ** -24)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bond_at_its_rest_length(pkg, dtype):
    case = R.exact_bond()
    s = case.system(pkg, dtype)
    assert np.all(pkg.forces(s, pairwise=False) == 0.0) and pkg.potential_energy(s, pairwise=False) == 0.0
    assert np.all(pkg.virial(s, pairwise=False, general=False) == 0.0)


# ---- d. the per-atom sums ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,mixed", [(m, False) for m in R.HUB_M] + [(m, True) for m in R.HUB_M_MIXED])
def test_hub_atom_slot_sums(pkg, m, mixed, dtype):
    """one atom in m slots (eight lanes per atom, 32 slots per round of the collect loop: below, at and over one, two and three rounds), a third of the atoms in no
    term at all; the mixed systems also at m = 11, the fewest slots with the hub in every role of every type.  Bonded forces per atom against the oracle; term-less atoms exactly zero, and in the full force call bit-identical to a system without terms; the
    evaluation repeats bit for bit."""
    case = R.hub(m, mixed, seed=0)
    free = np.arange(case.n_with_terms, case.n)
    assert case.slots[0] == m and 3 * len(free) >= case.n - 2 and case.n % 32 != 0
    s, f = check(pkg, "hub_mixed" if mixed else "hub_bonds", case, dtype)
    assert np.all(f[free] == 0.0)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    full = pkg.forces(s)
    assert np.array_equal(pkg.forces(s).view(bits), full.view(bits))
    bare = R.only(case)                                                     # the same atoms, pair exclusions and interactions; no specific interaction
    full_bare = pkg.forces(bare.system(pkg, dtype))
    assert np.abs(full_bare[free]).max() > 0
    assert np.array_equal(full[free].view(bits), full_bare[free].view(bits))
    assert not np.array_equal(full[0], full_bare[0])


# ---- e. after a re-sort ----------------------------------------------------------------------------------------------
def sorted_order(pkg, s, n):
    perm = np.empty(n, np.int32)
    s._check(pkg.lib().mhip_export_order(s.engine(), perm.ctypes.data_as(C.c_void_p), n))
    return perm


@pytest.mark.parametrize("dtype", DTYPES)
def test_terms_follow_the_atoms_through_a_re_sort(pkg, dtype):
    """terms address atoms through inv[]: after the chains' coordinates have been handed round among the chains the sorted order is another one, and every term
    must find its atoms where they are now"""
    case = R.chains(40, 40, 40, 40, seed=0)
    s = case.system(pkg, dtype)
    pkg.forces(s)                                                           # (the pair pass sorts the atoms)
    order0 = sorted_order(pkg, s, case.n)
    assert np.array_equal(np.sort(order0), np.arange(case.n)) and not np.array_equal(order0, np.arange(case.n))
    moved = R.regular_groups(0)["resort"][0]
    assert not np.array_equal(moved.coords, case.coords) and np.array_equal(np.sort(moved.coords, axis=0), np.sort(case.coords, axis=0))
    s.coords = moved.coords.astype(dtype)
    pkg.forces(s)                                                           # new coordinates: searched and sorted again
    order1 = sorted_order(pkg, s, case.n)
    assert np.array_equal(np.sort(order1), np.arange(case.n)) and not np.array_equal(order0, order1)
    check(pkg, "resort", moved, dtype, s=s)
    assert np.array_equal(sorted_order(pkg, s, case.n), order1)


# ---- f. the launch shapes of a run -------------------------------------------------------------------------------------
SHAPES = {   # kind, dtype, MOLLYHIP_FUSE_GATHER_VV, what the stats must show
    "pair_launch_terms": ("rf", np.float32, None, lambda st: st["n_group_split_passes"] > 0 and st["n_fused_steps"] == 0),
    "pme_spread_and_collect": ("pme", np.float32, "0", lambda st: st["n_group_split_passes"] > 0 and st["n_fused_steps"] == 0),
    "pme_integrating_launch": ("pme", np.float32, "1", lambda st: st["n_group_split_passes"] > 0 and st["n_fused_steps"] > 0),
    "fp64_own_grid": ("rf", np.float64, None, lambda st: st["n_group_split_passes"] == 0 and st["n_fused_steps"] == 0),
    "fp64_pme": ("pme", np.float64, "0", lambda st: st["n_group_split_passes"] == 0 and st["n_fused_steps"] == 0),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_launch_shapes_of_a_run(pkg, monkeypatch, shape):
    """Chains in a small argon fluid, at rest, RUN_STEPS velocity-Verlet steps (the fewest after which the stats show every path): from rest a velocity is a sum of
    forces times dt/2m, so a wrong bonded force on one atom shows in that atom's velocity.  7 term blocks and no exclusions: the launches that round up to four term
    blocks per workgroup (k_spread_bonded, the term workgroups of the group-split pair launch) run an idle one through the exclusion branch with null arrays.  The
    engine takes the group-split launch at this size by itself.  Velocities per atom against the fp64 oracle's run, measured against V_i
    (bonded_ref.velocity_scale): fp64 1e-9, fp32 twice what the oracle's own fp32 run loses (YARD32_RUN).  fp64 with PME runs k_spread_bonded and k_gather_collect in
    double."""
    kind, dtype, fuse, taken = SHAPES[shape]
    monkeypatch.delenv("MOLLYHIP_GROUP_SPLIT", raising=False)
    if fuse is None: monkeypatch.delenv("MOLLYHIP_FUSE_GATHER_VV", raising=False)
    else: monkeypatch.setenv("MOLLYHIP_FUSE_GATHER_VV", fuse)
    case = R.fluid_with_chains(kind)
    s = case.system(pkg, dtype)
    pkg.simulate(s, pkg.VelocityVerlet(dt=R.RUN_DT), RUN_STEPS)
    st = s.stats()
    print(f"[bonded] run {shape}: group_split {st['group_split']}, group-split passes {st['n_group_split_passes']}, integrating launches {st['n_fused_steps']}")
    assert taken(st), st
    scale = R.velocity_scale(case, RUN_STEPS)
    assert np.all(scale > 0)                                                # every atom is compared
    r = np.linalg.norm(np.asarray(s.velocities, dtype=np.float64) - R.oracle_run(case, np.float64, RUN_STEPS), axis=1) / scale
    bar = 1e-9 if dtype == np.float64 else 2.0 * YARD32_RUN[kind]
    print(f"[bonded] run {shape}: worst ‖Δv_i‖/V_i {r.max():.3e} (atom {int(r.argmax())}; chains only {r[case.n_fluid:].max():.3e}), bar {bar:.3e}")
    assert np.isfinite(r).all() and r.max() <= bar
