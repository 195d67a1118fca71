"""The list-lifetime contracts of the drop-in boundary and of the benchmarked kernel variant, on the GPU through the C ABI.

* `mhip_set_state` with unchanged topology refreshes coordinates WITHOUT throwing the pair lists away — the four-function drop-in path
  (set_state → forces(step_n) per step, as the stock `simulate!` loop drives `pairwise_forces_loop_gpu!`, ext/MollyCUDAExt.jl:774-783)
  must not re-sort and re-search at every call;
* the uniform-LJ fp32 prune emitter (the variant `bench.py` times) keeps the exported list bit-identical to a fresh reference search;
* velocity Verlet with massless atoms (calc_accels = 0 for m = 0, src/force.jl:17);
* a run cut into chunks repeats the uncut run with exact `==` (test/simulation.jl:16-57).
"""
import ctypes as C

import numpy as np
import pytest

from tests import systems as S

pytestmark = pytest.mark.gpu


def export_list(pkg, s):
    L = pkg.lib()
    n = C.c_int64(0)
    s._check(L.mhip_export_neighbors(s.engine(), None, None, None, 0, C.byref(n)))
    i = np.empty(n.value, np.int32); j = np.empty(n.value, np.int32); sp = np.empty(n.value, np.uint8)
    s._check(L.mhip_export_neighbors(s.engine(), s._ptr(i), s._ptr(j), s._ptr(sp), n.value, C.byref(n)))
    return S.sorted_pairs(i, j, sp)


@pytest.mark.parametrize("maker,dtype", [("lj", np.float32), ("lj", np.float64), ("charged", np.float32)])
def test_set_state_then_forces_every_step_keeps_the_lists(pkg, maker, dtype):
    """30 consecutive steps driven from the HOST: integrate on the CPU side (the oracle's velocity Verlet), hand the coordinates over
    with set_state, ask for forces(step_n).  Forces stay at oracle parity at every step while the engine searches at most twice and
    prunes a handful of times — not 30 sorts + searches."""
    case = S.lj_fluid(16, dtype=dtype) if maker == "lj" else S.charged_fluid(14, dict(kind="rf", rc=1.0), dtype=dtype, stable=True)
    s = case.system(pkg, dtype)
    o = case.oracle(np.float64)
    dt = 0.002 if maker == "lj" else 0.0005
    worst = 0.0
    for step in range(0, 31):
        if step:
            o.vv_run(1, dt, first_step=step - 1, remove_cm_every=1)      # one reference step on the host
        x = o.coords.copy()
        s.coords[:] = x.astype(dtype)
        f = pkg.forces(s, step_n=step).astype(np.float64)              # push_state → mhip_set_state → mhip_forces(step_n)
        oo = case.oracle(np.float64, coords=s.coords.astype(np.float64))
        f_ref = oo.forces(oo.neighbors("cell", nthreads=4), nthreads=4)
        err = np.linalg.norm(f - f_ref, axis=1).max() / np.linalg.norm(f_ref, axis=1).max()
        worst = max(worst, err)
        assert err < (1e-9 if dtype == np.float64 else 2e-4), f"step {step}: relative force error {err:.3e}"
    st = s.stats()
    # the argon fluid moves 0.05 nm in 30 steps: the first search (+ at most one more); the charged lattice is far from equilibrium
    # and its light atoms cover the 0.2 nm margin in about ten steps — still a fraction of one search per step
    assert st["n_outer_builds"] <= (2 if maker == "lj" else 5), st
    assert st["n_outer_builds"] + st["n_filter_passes"] <= (8 if maker == "lj" else 14), st
    assert st["n_force_calls"] >= 31


def test_set_state_with_far_moved_coordinates_searches_again(pkg):
    """the safety side of the same contract: coordinates that moved further than the lists' margins allow must trigger a new search"""
    case = S.lj_fluid(12, dtype=np.float64)
    s = case.system(pkg, np.float64)
    pkg.forces(s)
    n0 = s.stats()["n_outer_builds"]
    rng = np.random.default_rng(3)
    x2 = case.coords + rng.normal(size=case.coords.shape) * 0.3
    x2 -= np.floor(x2 / case.box) * case.box
    keep = np.ones(case.n, bool)      # avoid overlapping atoms: pull apart any pair closer than 0.25 nm by dropping the move
    oo = case.oracle(np.float64, coords=x2)
    i, j, _ = oo.neighbors("cell")
    d = x2[i] - x2[j]; d -= np.round(d / case.box) * case.box
    close = np.linalg.norm(d, axis=1) < 0.25
    keep[i[close]] = False; keep[j[close]] = False
    x2 = np.where(keep[:, None], x2, case.coords)
    s.coords[:] = x2
    oo = case.oracle(np.float64, coords=x2)
    f_ref = oo.forces(oo.neighbors("cell"))
    f = pkg.forces(s, step_n=1)
    assert np.abs(f - f_ref).max() <= 1e-9 * np.abs(f_ref).max() + 1e-8
    assert s.stats()["n_outer_builds"] == n0 + 1


def test_uniform_lj_fp32_dual_list_stays_bit_exact(pkg):
    """the one-type fp32 LJ fluid takes the hand-packed pair loop whose PRUNE instantiation emits the inner list (kernels.h, walk_rows):
    after 60 steps — prunes included — the list handed out equals a fresh fp32 reference search of the coordinates the engine holds"""
    case = S.lj_fluid(20, dtype=np.float32)
    s = case.system(pkg, np.float32)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002), 60)
    st = s.stats()
    assert st["minimg_mode"] == 0 and st["n_filter_passes"] >= 1, st      # block-local coordinates, the dual list really pruned
    got = export_list(pkg, s)
    o = case.oracle(np.float32, coords=s.coords.astype(np.float64))
    want = S.sorted_pairs(*o.neighbors("cell", nthreads=4))
    assert len(got[0]) == len(want[0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # and the forces of that state against the fp64 oracle at the fp32 bar
    tol, o64, nl = S.fp32_force_tolerance(case, coords=s.coords.astype(np.float64))
    f_ref = o64.forces(nl, nthreads=4)
    err = np.linalg.norm(pkg.forces(s, step_n=60).astype(np.float64) - f_ref, axis=1)
    S.fp32_check(err, tol)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_velocity_verlet_with_massless_atoms(pkg, dtype):
    """calc_accels is 0 for m = 0 (src/force.jl:17): massless atoms coast with their initial velocity, take part in the pair forces on
    the others, and carry no weight in remove_CM_motion!"""
    case = S.lj_fluid(8, dtype=dtype)
    mass = case.mass.copy(); mass[::7] = 0.0
    case.mass = mass
    o = case.oracle(np.float64)
    o.vv_run(25, 0.002, remove_cm_every=1)
    s = case.system(pkg, dtype)
    v0 = s.velocities.copy()
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002), 25)
    d = s.coords.astype(np.float64) - o.coords
    d -= np.round(d / case.box) * case.box
    if dtype == np.float64:
        assert np.abs(d).max() < 1e-10 and np.abs(s.velocities - o.vel).max() < 1e-9
    else:
        assert np.abs(d).mean() < 1e-5 and np.abs(d).max() < 1e-3
    # massless atoms: only the centre-of-mass corrections touched their velocities
    dv = (s.velocities[::7].astype(np.float64) - v0[::7].astype(np.float64))
    assert np.abs(dv - dv.mean(axis=0)).max() < (1e-12 if dtype == np.float64 else 1e-5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunked_continuation_is_exact_without_cm_removal(pkg, dtype):
    """test/simulation.jl:16-57 asserts `==` between 10 steps and 3 + 3 + 4 steps.  With the lists kept across chunk starts and the
    integrator's arithmetic shared by all its kernels, the chunked run walks the same lists in the same order: exact equality, when no
    centre-of-mass removal is pending across a chunk boundary (the fused integrator applies it one launch late, which rounds
    differently from applying it at the end of a chunk — see test_chunked_continuation for that case, at rounding level)."""
    case = S.lj_fluid(10, dtype=dtype)
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=0)
    a = case.system(pkg, dtype)
    pkg.simulate(a, sim, 10)
    b = case.system(pkg, dtype)
    pkg.simulate(b, sim, 3)
    pkg.simulate(b, sim, 3, init_step=3)
    pkg.simulate(b, sim, 4, init_step=6)
    assert np.array_equal(a.coords, b.coords) and np.array_equal(a.velocities, b.velocities)
    # 25 steps cut at 7 and 14 (the rebuild steps 10 and 20 fall inside chunks)
    a = case.system(pkg, dtype); pkg.simulate(a, sim, 25)
    b = case.system(pkg, dtype)
    for first, n in ((0, 7), (7, 7), (14, 11)):
        pkg.simulate(b, sim, n, init_step=first)
    assert np.array_equal(a.coords, b.coords) and np.array_equal(a.velocities, b.velocities)


def test_full_size_1m_lj_against_oracle(pkg):
    """BASELINE.json configs[3] on one GPU — the system `bench.py` times: 1 000 000-atom LJ fluid, fp32, forces against the fp64 oracle
    at the fp32 bar, Newton's third law, full list = 2 × the fp32 reference's half list."""
    case = S.lj_fluid(100, seed=4, dtype=np.float32)
    tol, o, nl = S.fp32_force_tolerance(case)
    f_ref = o.forces(nl, nthreads=16)
    s = case.system(pkg, np.float32)
    f = pkg.forces(s).astype(np.float64)
    err = np.linalg.norm(f - f_ref, axis=1)
    S.fp32_check(err, tol, "fp32 forces of the 1M-atom fluid against the fp64 oracle")
    assert S.rel_rms(err, f_ref) <= 1e-5
    assert np.abs(f.sum(axis=0)).max() < 1e-6 * o.pair_force_scale.sum()
    st = s.stats()
    o32 = case.oracle(np.float32)
    oi, oj, _ = o32.neighbors("cell", nthreads=16)
    assert st["n_pairs_full"] == 2 * len(oi)
    assert st["minimg_mode"] == 0 and st["block_atoms"] * st["j_split"] <= 1024
    keys, n_special = S.export_keys(pkg, s)                      # 76 M pairs: the same SET as the fp32 reference search
    assert n_special == 0 and np.array_equal(keys, S.pair_keys(oi, oj))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_new_velocities_on_old_coordinates_are_looked_at_before_the_lists_are_trusted(pkg, dtype):
    """A velocity-only change between two runs (re-thermalisation, a temperature ramp, a replica-exchange swap): the inner pair list was
    pruned with a skin sized for the speeds of the run before.  The continuation must check the new speeds at its first step — not at
    the next cadence step — and still follow the reference, which searches afresh at the start of every simulate! (simulators.jl:564).
    Handing the SAME state back, on the other hand, changes nothing: the chunked run stays bit-identical to the uncut one."""
    case = S.lj_fluid(14, dtype=dtype)
    dt = 0.002
    s = case.system(pkg, dtype)
    pkg.simulate(s, pkg.VelocityVerlet(dt=dt, remove_CM_motion=0), 13)             # ends off the cadence (13 % 10 != 0), lists alive
    n_outer = s.stats()["n_outer_builds"]
    o = case.oracle(np.float64, coords=s.coords.astype(np.float64), velocities=s.velocities.astype(np.float64) * 6.0)
    s.velocities[:] = (s.velocities.astype(np.float64) * 6.0).astype(dtype)      # 36x the temperature: 0.1 nm of inner skin goes in a few steps
    pkg.simulate(s, pkg.VelocityVerlet(dt=dt, remove_CM_motion=0), 12, init_step=13)
    o.vv_run(12, dt, first_step=13, remove_cm_every=0)
    d = s.coords.astype(np.float64) - o.coords
    d -= np.round(d / case.box) * case.box
    assert np.abs(d).max() < (2e-4 if dtype == np.float32 else 1e-8), np.abs(d).max()    # a pair lost from the list shows as 1e-2 nm here
    assert s.stats()["n_outer_builds"] + s.stats()["n_filter_passes"] > n_outer + 1          # the hot atoms forced list work
    # unchanged state handed back: no search, no prune, same bits
    a = case.system(pkg, dtype); b = case.system(pkg, dtype)
    pkg.simulate(a, pkg.VelocityVerlet(dt=dt, remove_CM_motion=0), 16)
    pkg.simulate(b, pkg.VelocityVerlet(dt=dt, remove_CM_motion=0), 7)
    before = b.stats()
    pkg.simulate(b, pkg.VelocityVerlet(dt=dt, remove_CM_motion=0), 9, init_step=7)
    after = b.stats()
    assert np.array_equal(a.coords, b.coords) and np.array_equal(a.velocities, b.velocities)
    assert after["n_outer_builds"] == before["n_outer_builds"]


def test_a_continued_run_finds_its_first_forces_already_there(pkg):
    """simulate!(sys, sim, n) recomputes the forces of its first step (simulators.jl:564-571); a run that continues from exactly the
    state the previous one left — same coordinates, same order, same lists — gets the same numbers from the force array of that run's
    last step.  Anything that could change them (new coordinates, a search, a prune) makes the first pass happen as before."""
    case = S.lj_fluid(12, dtype=np.float32)
    a = case.system(pkg, np.float32)
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=0)    # (with it a chunk end applies v_cm at another point of the launch sequence: equal to rounding only)
    pkg.simulate(a, sim, 7)
    c0 = a.stats()["n_force_calls"]
    pkg.simulate(a, sim, 6, init_step=7)                      # steps 8 … 13: the pass at the start is not needed
    c1 = a.stats()["n_force_calls"]
    assert c1 - c0 <= 6 + 1 and c1 - c0 >= 6                 # (+1 only if step 10's check asked for a second pass)
    b = case.system(pkg, np.float32)
    pkg.simulate(b, sim, 13)
    assert np.array_equal(a.coords, b.coords) and np.array_equal(a.velocities, b.velocities)   # bit for bit the uncut run
    # new coordinates: the forces of the first step are computed again
    a.coords = a.coords + np.float32(1e-4)
    c2 = a.stats()["n_force_calls"]
    pkg.simulate(a, sim, 3, init_step=13)
    assert a.stats()["n_force_calls"] - c2 >= 4


def test_terms_added_between_two_runs_count_from_the_first_step(pkg):
    """a run, then bonds added, then the run continued: the continued run must not take the previous run's last forces for its first
    step (they lack the new terms) — same trajectory as a system that had the bonds from the start of the second leg"""
    case = S.lj_fluid(10, dtype=np.float64)
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=0)
    a = case.system(pkg, np.float64)
    pkg.simulate(a, sim, 7)
    x7, v7 = a.coords.copy(), a.velocities.copy()
    n = case.n
    bi, bj = np.arange(0, n - 1, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    bk, br = np.full(n // 2, 3.0e4), np.full(n // 2, 0.35)
    a.specific_inter_lists = (pkg.HarmonicBonds(bi, bj, bk, br),)
    a._check(pkg.lib().mhip_set_bonds(a.engine(), len(bi), a._ptr(bi), a._ptr(bj), a._ptr(bk), a._ptr(br)))      # straight through the C ABI, as a Julia caller would
    pkg.simulate(a, sim, 5, init_step=7)
    b = S.Case(x7, case.box, lj=case.lj, r_list=case.r_list, rebuild_every=case.rebuild_every, velocities=v7, sigma=case.sigma, eps=case.eps, mass=case.mass,
               bonds=dict(i=bi, j=bj, k=bk, r0=br)).system(pkg, np.float64)
    pkg.simulate(b, sim, 5, init_step=7)
    assert np.abs(a.coords - b.coords).max() < 1e-9 and np.abs(a.velocities - b.velocities).max() < 1e-7



@pytest.mark.parametrize("remove_cm", [0, 1, 3])
def test_fused_step_repeats_the_separate_integrator_bit_for_bit(pkg, remove_cm, monkeypatch):
    """Inside mhip_vv_run the plain pair passes of the fp32 one-type fluids integrate in their own epilogue (kernels.h, the STEP variants: no force array, no
    integrator launch).  Same arithmetic, same order of the Σ m v partial sums (row sums by DPP in the association of the integrator kernels' butterfly), the
    centre-of-mass velocity subtracted one launch late in both: 120 steps — outer searches, prunes and validity checks included, which take the separate
    integrator either way — end in the SAME bits with the fused step on and off."""
    case = S.lj_fluid(40, seed=2, dtype=np.float32)      # 64 000 atoms: the packed loop and the dual list, as in the benchmarks
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=remove_cm)
    out = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("MOLLYHIP_FUSE_STEP", fuse)      # (read when the engine is created)
        s = case.system(pkg, np.float32)
        pkg.simulate(s, sim, 60)
        pkg.simulate(s, sim, 60, init_step=60)
        st = s.stats()
        assert (st["n_fused_steps"] > 60) == (fuse == "1"), st["n_fused_steps"]
        out.append((s.coords.copy(), s.velocities.copy()))
        s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_fused_step_trajectory_vs_fp64_oracle(pkg, slack):
    """The timed kernel of both LJ headlines, directly against the oracle: 100 steps of the 64 000-atom fp32 fluid through mhip_vv_run — packed loop, dual
    list, the pair pass integrating in its epilogue on every plain step (k_forces STEP) — against 100 steps of the fp64 oracle from the same start, at the
    reference's own fp32 trajectory bar: mean |Δx| < 5e-4 nm after 100 steps (test/simulation.jl:625).  The force parity tests hold the forces at the
    coordinates reached; this one holds the integration that reaches them.  The run is deterministic (no atomics on the LJ fluid's path), so the bars sit
    at 3× what round 6 measured (profiles/r06_tolerance_slack.jsonl: mean 2.5e-6 nm, worst 1.28e-5 nm, worst velocity 1.09e-4 nm/ps), not at the reference's 5e-4."""
    case = S.lj_fluid(40, seed=2, dtype=np.float32)
    s = case.system(pkg, np.float32)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002, remove_CM_motion=1), 100)
    st = s.stats()
    assert st["n_fused_steps"] > 60, st["n_fused_steps"]
    o = case.oracle(np.float64)
    o.vv_run(100, 0.002, remove_cm_every=1, nthreads=8)
    d = s.coords.astype(np.float64) - o.coords
    d -= np.round(d / case.box) * case.box
    dev = np.linalg.norm(d, axis=1)
    slack("mean coordinate deviation after 100 fused steps, nm (reference bar 5e-4: test/simulation.jl:625)", dev.mean(), 7.5e-6)
    slack("worst coordinate deviation after 100 fused steps, nm", dev.max(), 3.8e-5)
    dv = np.linalg.norm(s.velocities.astype(np.float64) - o.vel, axis=1)
    slack("worst velocity deviation after 100 fused steps, nm/ps", dv.max(), 3.2e-4)


def test_fused_step_without_a_j_split(pkg):
    """256-atom blocks WITHOUT a j-split (mhip_set_launch_config(256, 1)): the STEP epilogue's block sums of Σ m v land in LDS that the tile still occupies, and
    with no j-split reduction in between there was no barrier behind the row walk (round-5 advisor finding: a fast wave's sums could overwrite tile
    coordinates a slower wave of the block was still gathering).  With the centre of mass removed at every step the fused run must equal the
    separate-integrator run bit for bit, as in every other shape."""
    case = S.lj_fluid(40, seed=2, dtype=np.float32)
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=1)
    out = []
    import os
    for fuse in ("1", "0"):
        os.environ["MOLLYHIP_FUSE_STEP"] = fuse
        try:
            s = case.system(pkg, np.float32)
            pkg.set_launch_config(s, 256, 1)
            pkg.simulate(s, sim, 60)
            st = s.stats()
            assert st["block_atoms"] == 256 and st["j_split"] == 1, st
            assert (st["n_fused_steps"] > 30) == (fuse == "1"), st["n_fused_steps"]
            out.append((s.coords.copy(), s.velocities.copy()))
            s.close()
        finally:
            os.environ.pop("MOLLYHIP_FUSE_STEP", None)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    o = case.oracle(np.float64)
    o.vv_run(60, 0.002, remove_cm_every=1, nthreads=8)
    d = out[0][0].astype(np.float64) - o.coords
    d -= np.round(d / case.box) * case.box
    assert np.linalg.norm(d, axis=1).mean() < 5e-4
