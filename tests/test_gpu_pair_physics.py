"""The nonbonded pair physics, pair by pair: every implementation of the pair arithmetic (pair_eval / pair_eval2 of csrc/physics.h, the row walkers of
k_forces, the one-type loops of forces_uniform.hip, the step-loop variants) against the plain restatement tests/pair_ref.py at longdouble, on systems of
ISOLATED DIMERS (pair_ref.probe_system): every atom has one partner, so the force on it is one pair's force and an error belongs to one pair.  The dimers
sit in the core, the well, mid-range, a relative δ (2⁻¹⁶ fp32, 2⁻⁴⁰ fp64) on either side of every activation and cutoff radius, inside the switch, between
cutoff and list radius, and beyond the list; crossed with species that switch one interaction off each and with plain / special / excluded pairs.  The
dense-fluid tests cannot see a `<` for a `<=` (tests/systems.py:fp32_force_tolerance allows the jump of every near-cutoff pair) — these can.

Bars, from the reference's own arithmetic (computed here on the CPU, per case; pair_ref.reference_errors): E32 / E64 = the worst
|pair_ref(fp32 / fp64) − pair_ref(longdouble)|/S over the case's dimers, S = 24ϵ(2s¹² + s⁶)/r + |kqq|/r² the pair's bare magnitude, times
    fp64 kernels                    4   (set out as 16: device exp / erfc are not correctly rounded, contraction differs; measured 0.16 of that bar: tightened)
    fp32 one-partner paths          4   v_rcp / v_rsq / v_sqrt / v_exp are 1-ulp units
    fp32 packed loop (pair_eval2)   8   one v_rcp of a product serves two partners, exp2 takes a pre-multiplied constant
— and, never wider than that, the same factor on the pair formula's arithmetic alone plus ONE rounding of a coordinate at the size of the box, which is what
E32 mostly consists of (a dimer's bar is min(k·E·S, k·E_arith·S + D), D its own sensitivity to such a rounding).  Measured on the MI355X: the worst
dimer of any case uses 0.50 of its fp32 bar and 0.42 of its fp64 bar.  The dimers AT a radius (grid systems) have exact displacements: k/2·E_arith (fp32), k/4 (fp64).
Energy and virial always take the one-partner arithmetic (ENERGY = true → pair_eval); each distance class is a system of its own so that an edge class is not
drowned by the core dimers, and the totals are held to the SUM of the dimers' bars with factor 1 (set out as 4 / 16; measured 0.11 / 0.03 of that: the errors
of independent pairs add in quadrature, their worst cases linearly) plus what the double-precision sums over the atoms may round.  tests/test_pair_host.py validates pair_ref and the probe systems without a GPU."""
import numpy as np
import pytest

from tests import pair_ref as R
from tests import systems as S

pytestmark = pytest.mark.gpu

IDS = [f"{n}-{np.dtype(d).name}" for n, d in R.GPU_CASES]
PACKED = ("rf", "rf_inf", "ewald", "small_rf", "small_ewald", "tri_rf_approx", "tri_rf_images", "tri_ewald_approx", "tri_ewald_images")
# fp32, LJ DistanceCutoff + reaction field / A&S Ewald, ONE cutoff: k_forces walks the rows two partners at a time (kernels.h PK2).  The exact-erfc Ewald and the
# two-cutoff launches (Pk2Consts::usable) keep the one-partner loop, and so does any row that holds a special pair.


def factor(name, dtype, special):
    """how many E the path that evaluates these dimers' forces is allowed (the table above), as an array over the dimers"""
    if np.dtype(dtype) == np.float64:
        return np.full(len(special), 4.0)
    return np.where(special, 4.0, 8.0) if name in PACKED else np.full(len(special), 4.0)


def check_path(name, dtype, st, case, minimg=None):
    """the variant this case is meant to reach really ran; minimg: the expected minimg_mode (None: whichever the engine chose — printed)"""
    print(f"[layout] {name} {np.dtype(dtype).name}: n {case.n}, block_atoms {st['block_atoms']}, j_split {st['j_split']}, blocks {st['n_blocks']}, minimg_mode {st['minimg_mode']}, "
          f"group_split {st['group_split']}, gs passes {st['n_group_split_passes']}, fused steps {st['n_fused_steps']}, prunes {st['n_filter_passes']}, list slots {st['n_list_slots']}")
    assert st["n_atoms"] == case.n
    if name.startswith("small"):
        assert st["minimg_mode"] == 1 and st["n_blocks"] == 1, st            # one block spans the box: the exact minimum image inside the loop
    elif minimg is not None:
        assert st["minimg_mode"] == minimg, st


def expected_minimg(name):
    """1 024 atoms in 16 blocks of a 20.8 nm box: the image is resolved when the tile is staged (block-local coordinates).  The NoCutoff systems are 250 atoms in
    4 blocks of a 13 nm box — a block spans more than half of it, so they take the in-loop image like the small boxes; a triclinic box may take either."""
    return None if name.startswith("tri") else (1 if name.endswith("_none") else 0)


def check_forces(name, dtype, p, f, slack, extra=0.0, tag="forces"):
    grid = getattr(p, "arith_from", None) is not None
    """per dimer atom against pair_ref at longdouble, Newton's third law within the dimer, exact zeros, no non-finite component anywhere"""
    err = R.reference_errors(p, dtype)
    hi = err["ref"]
    f = np.asarray(f, dtype=np.float64)
    assert np.isfinite(f).all(), f"{int((~np.isfinite(f)).sum())} non-finite force components"
    S_ = err["S"]
    f_ref = np.asarray(hi["f"], dtype=np.float64)
    zero = R.structural_zero(p)
    bad = zero & ((f[p.ia] != 0).any(axis=1) | (f[p.ib] != 0).any(axis=1))
    assert not bad.any(), f"{int(bad.sum())} dimers that must feel exactly nothing carry a force: classes {sorted(set(p.cls[bad]))}, flags {sorted(set(p.flag[bad]))}, worst {np.abs(f[p.ib][bad]).max():.3e}"
    live = ~zero & (S_ > 0)
    k = factor(name, dtype, p.flag == "special") * ((0.25 if np.dtype(dtype) == np.float64 else 0.5) if grid else 1.0)
    bar = err["bar_f"](k) + extra * S_
    d_j = np.linalg.norm(f[p.ib] - f_ref, axis=1)
    d_i = np.linalg.norm(f[p.ia] + f_ref, axis=1)
    d_n = np.linalg.norm(f[p.ia] + f[p.ib], axis=1)
    for what, d in (("force on j", d_j), ("force on i", d_i), ("Newton's third law", d_n)):
        ratio = d[live] / bar[live]
        w = int(np.argmax(ratio))
        cls, fl = p.cls[live][w], p.flag[live][w]
        slack(f"{tag}: {what}, worst error / bar(k), k = {sorted(set(k.tolist()))} (class {cls}, {fl})", float(ratio.max()), 1.0)
    # the probes just inside a jump carry their force (the bar above) and that force is no rounding artefact: ≥ 100× the bar 
    j = R.jump_probes(p)
    if j.any():
        assert j.sum() >= 2 and np.all(np.linalg.norm(f_ref[j], axis=1) >= 100 * bar[j])
        assert np.all(np.linalg.norm(f[p.ib][j], axis=1) > 0)
    return err


@pytest.mark.parametrize("name,dtype", R.GPU_CASES, ids=IDS)
def test_pair_forces(pkg, slack, name, dtype):
    p = R.probe(name, dtype)
    s = p.case.system(pkg, dtype)
    f = pkg.forces(s)
    check_path(name, dtype, s.stats(), p.case, expected_minimg(name))
    check_forces(name, dtype, p, f, slack)


@pytest.mark.parametrize("name,dtype", R.GPU_CASES, ids=IDS)
def test_pair_energy_and_virial(pkg, slack, name, dtype):
    """each distance class as its own system: Σ pair energies and the six components of Σ fr·dr⊗dr against pair_ref at longdouble"""
    k = 1.0
    worst_e = worst_w = 0.0
    for cl in R.probe(name, dtype).classes:
        re, rw, e, e_ref = energy_and_virial(pkg, R.probe(name, dtype, only=cl), dtype, k)
        print(f"[class] {name} {np.dtype(dtype).name} {cl}: energy {e:.9g} (ref {e_ref:.9g}, {re:.3f} of the bar), virial {rw:.3f} of the bar")
        assert re <= 1.0, f"class {cl}: energy {e!r} against {e_ref!r}, {re:.2f} of the bar"
        assert rw <= 1.0, f"class {cl}: virial {rw:.2f} of the bar"
        worst_e, worst_w = max(worst_e, re), max(worst_w, rw)
    slack(f"energy, worst class: |ΔE| / Σ bar_e({k:g})", worst_e, 1.0)
    slack(f"virial, worst class and component: |ΔW| / Σ bar_w({k:g})", worst_w, 1.0)


STEP_MASS, STEP_DT, N_STEPS = float(np.float32(1.0e12)), 0.001, 3      # (the mass as fp32 holds it)


def energy_and_virial(pkg, p, dtype, k):
    """(|ΔE| / bar, |ΔW| / bar, e, e_ref) of one probe system's totals against Σ pair_ref at longdouble; a system in which nothing interacts must give exactly 0"""
    err = R.reference_errors(p, dtype)
    hi = err["ref"]
    listed = hi["listed"]
    s = p.case.system(pkg, dtype)
    e, w = pkg.potential_energy(s), pkg.virial(s)
    e_ref, w_ref = float(hi["pe"].sum()), np.asarray(hi["vir"].sum(axis=0), dtype=np.float64)
    assert np.isfinite(e) and np.isfinite(w).all()
    if not np.any(np.asarray(hi["fr"], dtype=np.float64) != 0):
        assert e == 0.0 and np.all(w == 0.0), (e, w)
        return 0.0, 0.0, e, e_ref
    bar_e = float(err["bar_e"](k)[listed].sum()) + R.sum_allowance(hi["pe"])
    bar_w = float(err["bar_w"](k)[listed].sum()) + R.sum_allowance(hi["vir"].reshape(-1, 9))
    return abs(e - e_ref) / bar_e, float(np.abs(w - w_ref).max()) / bar_w, e, e_ref


@pytest.mark.parametrize("name,dtype", R.GRID_GPU_CASES, ids=[f"{n}-{np.dtype(d).name}" for n, d in R.GRID_GPU_CASES])
def test_pair_inclusion_at_exactly_the_cutoff(pkg, slack, name, dtype):
    """`r <= rc` includes r == rc.  Dimers whose distance IS the radius, on a binary grid where every step from coordinates to r² is exact in the kernel as in the
    reference (pair_ref.grid_probe_system): they carry the full force of the jump, their neighbours one grid step outside carry exactly nothing.  Forces, energy
    and virial; the probes a relative δ inside the radius (test_pair_forces) cannot tell `<` from `<=`, nor an off-by-one in the packed loop's rc²⁺."""
    p = R.grid_probe(name, dtype)
    s = p.case.system(pkg, dtype)
    f = pkg.forces(s)
    check_path(name, dtype, s.stats(), p.case, 0)      # (not the small boxes: check_path holds those to the in-loop image)
    check_forces(name, dtype, p, f, slack)
    re, rw, e, e_ref = energy_and_virial(pkg, p, dtype, 1.0)
    print(f"[grid] {name} {np.dtype(dtype).name}: energy {e:.9g} (ref {e_ref:.9g})")
    slack("energy of the dimers at the radius: |ΔE| / Σ bar_e", re, 1.0)
    slack("virial of the dimers at the radius: |ΔW| / Σ bar_w", rw, 1.0)


VV_CASES = [("rf", ""), ("ewald", ""), ("lj_uniform", ""), ("lj_uniform_special", ""), ("rf", "bonds"), ("ewald", "bonds"),
            ("rf", "grid"), ("ewald", "grid"), ("lj_uniform", "grid"), ("mismatch_rf", "grid"), ("rf", "grid_bonds"), ("ewald", "grid_bonds")]


@pytest.mark.parametrize("name,kind", VV_CASES, ids=[n + ("_" + k if k else "") for n, k in VV_CASES])
def test_pair_forces_through_velocity_verlet_steps(pkg, slack, monkeypatch, name, kind):
    """The step-loop variants of the pair pass — the PRUNE forms at the step that builds the list, the one-type fused step, the plain passes whose forces the
    last launch integrates, and the group-split pass (forces_gs.hip) — through three velocity-Verlet steps from rest with atoms so heavy that nothing moves
    (x + v·dt == x in fp32): every step sees the same pairs at the same distances and v(3dt) = 3·f·dt/m, so f = m·v/(3dt) is the force the steps saw, per atom.
    The same per-pair checks, with the kicks' roundings added to the bar: per step two products f·(dt/2m) and two sums, 12·2⁻²⁴ relative in all.
    `grid`: the dimers at exactly the cutoff radius.  `bonds`: the group-split pass runs only in steps that also have bonded terms to fold in
    (engine.hip:step_forces), so these cases give every dimer a harmonic bond of strength 0: the pairs stay isolated, the bonded force is exactly zero, and the
    launch is the one a solvated protein takes."""
    bonds = kind.endswith("bonds")
    dtype = np.float32
    p = R.grid_probe(name, dtype) if kind.startswith("grid") else R.probe(name, dtype)
    c = p.case
    monkeypatch.setenv("MOLLYHIP_GROUP_SPLIT", "4") if bonds else monkeypatch.delenv("MOLLYHIP_GROUP_SPLIT", raising=False)
    heavy = S.Case(c.coords, c.box, lj=c.lj, coul=c.coul, r_list=c.r_list, rebuild_every=c.rebuild_every, velocities=np.zeros((c.n, 3)), charge=c.charge, sigma=c.sigma,
                   eps=c.eps, mass=np.full(c.n, STEP_MASS), excluded=c.excluded, special=c.special, name=c.name + "_heavy",
                   bonds=dict(i=p.ia.astype(np.int32), j=p.ib.astype(np.int32), k=np.zeros(len(p.ia)), r0=np.full(len(p.ia), 0.3)) if bonds else None)
    s = heavy.system(pkg, dtype)
    x0 = np.array(s.coords, dtype=np.float64)
    pkg.simulate(s, pkg.VelocityVerlet(dt=STEP_DT, remove_CM_motion=0), N_STEPS)
    st = s.stats()
    check_path(name, dtype, st, c, expected_minimg(name))
    assert np.abs(np.asarray(s.coords, dtype=np.float64) - x0).max() < 1e-9           # nothing moved
    f = np.asarray(s.velocities, dtype=np.float64) * (STEP_MASS / (N_STEPS * STEP_DT))
    check_forces(name, dtype, p, f, slack, extra=12 * 2.0 ** -24, tag=f"{N_STEPS} VV steps")
    assert st["n_filter_passes"] >= 1, st                                              # step 0 pruned the list it had just searched: the PRUNE form computed its forces
    if bonds:
        assert st["group_split"] == 4 and st["block_atoms"] == 64 and st["j_split"] == 16 and st["n_group_split_passes"] >= 1, st
    elif name == "lj_uniform":
        assert st["n_fused_steps"] >= 1, st                                            # the one-type fused step (forces_uniform.hip, STEP)
    else:
        assert st["n_group_split_passes"] == 0, st
