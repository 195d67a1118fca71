"""mhip_minimize (csrc/minimize.hip, the loop in csrc/engine.hip): simulate!(sys, ::SteepestDescentMinimizer) (simulators.jl:183-271) inside the engine, against
the numpy loop of tests/minimize_ref.py, the loop over the oracle, and the host loop of api.py on the twin System that carries the constraints as bonds.

Every comparison first asserts on the REFERENCE run that no decision was close to a tie (|E_trial − E| above ten times the project's potential-energy bar for
the precision) and that both branches were taken at least twice; a reference run that fails this wants another input, never another bar."""
import ctypes as C

import numpy as np
import pytest

from tests import constraints_ref, minimize_ref as R, systems as S, virtual_sites_ref as V
from tests.test_gpu_boundary import make
from tests.test_gpu_triclinic import sheared_fluid

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -3
# ten times the potential-energy agreement bars of tests/test_gpu_parity.py (fp64: rel 1e-10, abs 1e-8) and tests/test_gpu_pme.py / test_gpu_parity.py (fp32: rel 2e-5)
TIE_REL = {np.float64: 1e-9, np.float32: 2e-4}
TIE_ABS = {np.float64: 1e-7, np.float32: 1e-7}
E_REL = {np.float64: 1e-9, np.float32: 2e-5}
# nm: fp64, the bar of test_steepest_descent_minimizer_follows_the_oracle.  fp32 against the same loop on the host started at the fp32 trajectory bar, 5e-5
# (test_gpu_boundary.py:252); each test now passes its own, at most 3× what it measured on the MI355X (recorded through `slack`)
X_BAR = {np.float64: 1e-9, np.float32: 5e-5}


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def engine_run(pkg, s, max_steps, step_size, tol=0.0, k=500_000.0, first=0, rc=0):
    """mhip_minimize on the System's context, the state pushed before and pulled after → (log4 rows of the steps taken, out8 as a dict)"""
    log4 = np.full((max(max_steps, 1), 4), np.nan); out8 = np.full(8, np.nan)
    s.push_state(velocities=True)
    got = pkg.lib().mhip_minimize(s._ctx, first, max_steps, step_size, tol, 0.0 if k is None else k, dptr(log4), dptr(out8))
    assert got == rc, pkg.lib().mhip_last_error(s._ctx).decode()
    s.pull_state()
    info = dict(zip(("E0", "E", "max_force", "hn", "steps", "accepted", "rejected", "converged"), out8.tolist()))
    return log4[: int(out8[4])] if rc == 0 else log4, info


def loop_over(pkg, s, max_steps, step_size, tol=0.0):
    """the numpy loop over the engine's one-shot calls on `s` (forces distributes the sites' rows); `s` ends at the loop's coordinates"""
    def at(x):
        s.coords[:] = x
        return s

    def place(x):
        pkg.place_virtual_sites(at(x))
        return s.coords.copy()
    out = R.loop(s.coords, lambda x: pkg.forces(at(x)), lambda x: pkg.potential_energy(at(x)), step_size, max_steps, tol, dtype=s.dtype,
                 wrap_fn=lambda x: pkg.wrap_coords(x, s.boundary), place_fn=place if s.virtual_sites else None)
    s.coords[:] = out["coords"]
    return out


def host_loop(pkg, s, max_steps, step_size, tol=0.0, init_step=0):
    """the host loop of api.py (engine_loop=False) with its log read back → the same record as R.loop's"""
    words = []

    class Log:
        def write(self, t):
            words.append(t)
    pkg.simulate(s, pkg.SteepestDescentMinimizer(step_size=step_size, max_steps=max_steps, tol=tol, log_stream=Log()), init_step=init_step)
    rows = [l.split() for l in "".join(words).splitlines() if l.startswith("Step")]
    E0 = float(rows[0][5]); E = E0
    out = dict(accepted=[], E_trial=[], max_force=[], E0=E0, coords=s.coords.copy())
    for r in rows[1:]:
        out["E_trial"].append(float(r[5])); out["max_force"].append(float(r[9])); out["accepted"].append(r[-1] == "accepted")
        if out["accepted"][-1]:
            E = out["E_trial"][-1]
    out["E"] = E
    return out


def well_separated(ref, dtype, need=2):
    """the precondition on the reference run: no step near a tie, both branches taken"""
    dtype = np.dtype(dtype).type
    E = ref["E0"]
    for n, (Et, acc) in enumerate(zip(ref["E_trial"], ref["accepted"])):
        margin = max(TIE_REL[dtype] * abs(E), TIE_ABS[dtype])
        assert abs(Et - E) > margin, f"reference step {n + 1}: |E_trial − E| = {abs(Et - E):.3g} is within the tie margin {margin:.3g}: change the input"
        if acc:
            E = Et
    assert sum(ref["accepted"]) >= need and len(ref["accepted"]) - sum(ref["accepted"]) >= need, ref["accepted"]


def agree(slack, name, dtype, s, log4, info, ref, x_ref, x32=None):
    dtype = np.dtype(dtype).type
    assert [bool(a) for a in log4[:, 2]] == ref["accepted"], (log4[:, 2].tolist(), ref["accepted"])
    box = np.asarray(s.boundary.side_lengths, dtype=np.float64)
    dx = np.asarray(s.coords, dtype=np.float64) - np.asarray(x_ref, dtype=np.float64)
    if not hasattr(s.boundary, "basis_vectors"):
        dx -= box * np.round(dx / box)      # (an atom that sits on the box face may wrap either way)
    slack(f"{name}: coordinates [nm]", np.abs(dx).max(), x32 if dtype is np.float32 and x32 else X_BAR[dtype])
    assert info["E"] == pytest.approx(ref["E"], rel=E_REL[dtype], abs=TIE_ABS[dtype])
    np.testing.assert_allclose(log4[:, 0], ref["E_trial"], rtol=10 * E_REL[dtype], atol=TIE_ABS[dtype])
    np.testing.assert_allclose(log4[:, 1], ref["max_force"], rtol=1e-9 if dtype is np.float64 else 1e-4)
    assert info["steps"] == len(ref["accepted"]) and info["accepted"] == sum(ref["accepted"]) and info["rejected"] == info["steps"] - info["accepted"]


# ---- 1. kernel edges ----------------------------------------------------------------------------------------------------------------------
def lj_cluster(n, first=None, seed=5):
    """n argon-like atoms on a jittered lattice of 0.39 nm in the middle of a 6 nm box, one atom pushed towards a neighbour; first: the atom that leads in caller order"""
    rng = np.random.default_rng(seed + n)
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    x = 3.0 - 0.5 * side * 0.39 + g * 0.39 + rng.uniform(-0.01, 0.01, (n, 3))
    if n > 2:
        x[1] += 0.06 * (x[0] - x[1]) / np.linalg.norm(x[0] - x[1])
    if first is not None:
        x = np.roll(x, -first, axis=0)
    return S.Case(x, 6.0, lj=dict(cutoff=("distance", 1.0)), r_list=1.2, rebuild_every=10, velocities=np.zeros((n, 3)), sigma=np.full(n, 0.34), eps=np.full(n, 0.997),
                  mass=np.full(n, 39.948), name=f"lj_cluster{n}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_atom_stops_converged_where_it_is(pkg, dtype):
    case = lj_cluster(1)
    s = case.system(pkg, dtype)
    x0 = s.coords.copy()
    log4, info = engine_run(pkg, s, 5, 0.01, tol=1.0)
    assert info["steps"] == 1 and info["converged"] == 1 and info["max_force"] == 0 and info["E0"] == 0 and info["E"] == 0
    assert np.array_equal(s.coords, x0) and log4[0, 2] == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_atoms_reach_the_lj_minimum(pkg, dtype):
    case = lj_cluster(2)
    case.coords[1] = case.coords[0] + [0.42, 0.0, 0.0]
    s = case.system(pkg, dtype)
    log4, info = engine_run(pkg, s, 400, 0.05, tol=1e-3)
    r = np.linalg.norm(np.asarray(s.coords[1] - s.coords[0], dtype=np.float64))
    # fp64: F = 57.1 ϵ/σ² · δr ≈ 493 δr < tol = 1e-3 leaves δr < 2e-6.  fp32: energies of ≈ 1 kJ/mol resolve to 6e-8, i.e. k/2 δr² down to δr ≈ 1.6e-5 nm
    assert abs(r - 2 ** (1 / 6) * 0.34) < (1e-5 if dtype is np.float64 else 1e-4), r
    assert info["E"] == pytest.approx(-0.997, rel=1e-6) and info["accepted"] >= 2 and info["rejected"] >= 2
    if dtype is np.float64:
        assert info["converged"] == 1 and info["max_force"] < 1e-3 and info["steps"] < 400


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", [63, 64, 65, 257, 1025])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lj_clusters_at_the_kernel_edges(pkg, slack, dtype, n, where):
    top = int(np.argmax(np.linalg.norm(pkg.forces(lj_cluster(n).system(pkg, np.float64)), axis=1)))
    case = lj_cluster(n, first=top if where == "first" else (top + 1) % n)      # the atom with the largest force leads, or closes, the caller's order
    assert int(np.argmax(np.linalg.norm(pkg.forces(case.system(pkg, np.float64)), axis=1))) == (0 if where == "first" else n - 1)
    # (step_size 0.5, 8 steps: in fp64 numpy over all pairs every size takes at least two steps back and keeps |ΔE| above 5e-4 |E|)
    ref = loop_over(pkg, (t := case.system(pkg, dtype)), 8, 0.5)
    well_separated(ref, dtype)
    s = case.system(pkg, dtype)
    log4, info = engine_run(pkg, s, 8, 0.5)
    agree(slack, f"lj cluster {n} {where}", dtype, s, log4, info, ref, t.coords, x32=2e-6)      # (measured: 2.4e-7 … 7.2e-7)


# ---- 2. charged fluid with PME and exception lists against the loop over the oracle ---------------------------------------------------------
def test_pme_fluid_follows_the_loop_over_the_oracle(pkg):
    case, dtype = make("pme_fp64")
    x0 = case.coords + np.random.default_rng(3).normal(scale=0.01, size=case.coords.shape)
    o = case.oracle(np.float64, coords=x0)
    full = dict(specific=True, general=True)

    def at(x):
        o.coords[:] = x
        return o
    ref = R.loop(x0, lambda x: at(x).forces(o.neighbors("cell", nthreads=8), nthreads=4, **full), lambda x: at(x).potential_energy(o.neighbors("cell", nthreads=8), **full),
                 0.05, 10, 0.0, box=case.box)      # (chosen on the CPU: five steps accepted, five taken back, every |ΔE| above 7 % of E)
    well_separated(ref, np.float64)
    s = case.system(pkg, dtype, coords=x0)
    log4, info = engine_run(pkg, s, 10, 0.05)
    assert [bool(a) for a in log4[:, 2]] == ref["accepted"]
    assert np.abs(s.coords - ref["coords"]).max() < 1e-9
    assert info["E"] == pytest.approx(ref["E"], rel=1e-9)
    # the records are consistent with each other and with the System afterwards
    acc = log4[:, 2] == 1
    assert info["E"] == log4[acc, 0][-1] and info["accepted"] == acc.sum() and info["rejected"] == (~acc).sum() and info["steps"] == 10 and info["converged"] == 0
    assert info["max_force"] == log4[-1, 1] and log4[0, 3] == 0.05
    hn = 0.05
    for row in log4:
        assert row[3] == hn
        hn = 6 * hn / 5 if row[2] else hn / 5
    assert info["hn"] == hn
    assert pkg.potential_energy(s) == pytest.approx(info["E"], rel=1e-12) and info["E"] < info["E0"]


# ---- 3. every cluster kind: the constraints as bonds, or ignored ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [500_000.0, None])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constraint_clusters_against_the_host_loop_on_the_twin(pkg, slack, dtype, k):
    case = constraints_ref.toy_system(4)
    rng = np.random.default_rng(8)
    x0 = case.coords + rng.normal(scale=0.004, size=case.coords.shape)      # (bonds off their lengths: the constraint bonds pull from the first step)
    step = 0.02 if k else 0.2      # (chosen over the oracle in fp64: three resp. two steps taken back in ten, every |ΔE| above 2e-3 |E|)
    t = R.twin_with_bonds(case, k).system(pkg, dtype, coords=x0)
    ref = host_loop(pkg, t, 10, step)
    well_separated(ref, dtype)
    s = case.system(pkg, dtype, coords=x0)
    assert s.constraints and not t.constraints
    log4, info = engine_run(pkg, s, 10, step, k=k)
    agree(slack, f"toy clusters k={k}", dtype, s, log4, info, ref, t.coords, x32=3.5e-6)      # (measured: 0 with the bonds, 1.2e-6 without)
    print(f"[minimize] toy clusters k={k} {np.dtype(dtype).name}: largest |r − d| after the run {R.pair_deviation(case, np.asarray(s.coords, dtype=np.float64)):.3e} nm (not enforced)")


def test_simulate_engine_loop_takes_a_constrained_system(pkg):
    """the Python mirror: engine_loop=True admits what the default path refuses, and prints the host loop's lines"""
    case = constraints_ref.toy_system(4)
    x0 = case.coords + np.random.default_rng(8).normal(scale=0.004, size=case.coords.shape)
    lines, want = [], []

    class Log:
        def __init__(self, to):
            self.to = to

        def write(self, t):
            self.to.append(t)
    s = case.system(pkg, np.float64, coords=x0)
    with pytest.raises(pkg.MollyHipError):
        pkg.simulate(s, pkg.SteepestDescentMinimizer(max_steps=3))
    pkg.simulate(s, pkg.SteepestDescentMinimizer(step_size=0.02, max_steps=6, tol=0.0, log_stream=Log(lines), engine_loop=True))
    t = R.twin_with_bonds(case, 500_000.0).system(pkg, np.float64, coords=x0)
    pkg.simulate(t, pkg.SteepestDescentMinimizer(step_size=0.02, max_steps=6, tol=0.0, log_stream=Log(want)))
    got, ref = "".join(lines).splitlines(), "".join(want).splitlines()
    assert len(got) == len(ref) == 7
    for a, b in zip(got, ref):
        a, b = a.split(), b.split()
        assert a[:5] == b[:5] and a[6:9] == b[6:9] and a[-1] == b[-1] and float(a[5]) == pytest.approx(float(b[5]), rel=1e-9)
    assert np.abs(s.coords - t.coords).max() < 1e-9


# ---- 4. virtual sites -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["toy", "tip4p"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_virtual_sites_are_spread_and_placed(pkg, slack, dtype, which):
    if which == "toy":      # all four site types, one of them hosted by no single item; no constraints
        case = V.toy_case(); step, n = 0.05, 10
        x0 = case.coords.copy()
    else:                   # 8 rigid four-site waters: sites and constraints together
        case = V.tip4p_box(2); step, n = 0.02, 10
        x0 = case.coords + np.random.default_rng(4).normal(scale=0.003, size=case.coords.shape)
    t = R.twin_with_bonds(case, 500_000.0).system(pkg, dtype, coords=x0)
    ref = loop_over(pkg, t, n, step)
    well_separated(ref, dtype)
    s = case.system(pkg, dtype, coords=x0)
    log4, info = engine_run(pkg, s, n, step)
    agree(slack, f"sites {which}", dtype, s, log4, info, ref, t.coords, x32=2.4e-7)      # (measured: 0; the bar is one fp32 ulp of a coordinate below 2 nm)
    placed = V.place(np.asarray(s.coords, dtype=np.float64), case.box, case.virtual_sites)
    d = placed - np.asarray(s.coords, dtype=np.float64)
    d -= case.box * np.round(d / case.box)
    assert np.abs(d).max() < (1e-12 if dtype is np.float64 else 2e-6)      # every site sits where place puts it (fp32: a few ulp of a coordinate of ≈ 1 nm)


# ---- 5. lists outrun mid-run ----------------------------------------------------------------------------------------------------------------
def test_lists_are_renewed_when_the_moves_outrun_the_skin(pkg):
    case = S.lj_fluid(12, dtype=np.float64, r_cut=1.0, r_list=1.05, jitter=0.05)
    s = case.system(pkg, np.float64)
    pkg.potential_energy(s)
    r0 = s.stats()["n_rebuilds"]
    log4, info = engine_run(pkg, s, 12, 0.02)
    acc = log4[:, 2] == 1
    assert log4[acc, 3].sum() > 0.05, "the accepted moves must add up to more than the skin: change the input"
    fresh = case.system(pkg, np.float64, coords=s.coords)
    assert pkg.potential_energy(fresh) == pytest.approx(info["E"], rel=1e-12)
    r1 = s.stats()["n_rebuilds"]
    assert r0 < r1 < r0 + info["steps"], (r0, r1)
    assert pkg.potential_energy(s) == pytest.approx(info["E"], rel=1e-12)      # … and the lists the context is left with are good for the coordinates it holds


# ---- 6. TriclinicBoundary ---------------------------------------------------------------------------------------------------------------------
def test_triclinic_fluid_against_the_host_loop(pkg, slack):
    basis, case = sheared_fluid(np.float64)
    x0 = case.coords + np.random.default_rng(6).normal(scale=0.01, size=case.coords.shape)
    t = case.system(pkg, np.float64, coords=x0)
    ref = host_loop(pkg, t, 8, 0.6)      # (over the oracle: the first and the sixth step are taken back, every |ΔE| above 2e-2 |E|)
    well_separated(ref, np.float64)
    s = case.system(pkg, np.float64, coords=x0)
    log4, info = engine_run(pkg, s, 8, 0.6)
    agree(slack, "triclinic fluid", np.float64, s, log4, info, ref, t.coords)


# ---- 7. around the call -----------------------------------------------------------------------------------------------------------------------
def test_velocities_two_calls_zero_steps_and_a_run_afterwards(pkg, slack):
    case = S.charged_fluid(8, dict(kind="ewald", rc=1.0, tol=5e-4), dtype=np.float32, pme=dict(order=5, error_tol=5e-4), stable=True)
    x0 = case.coords + np.random.default_rng(2).normal(scale=0.005, size=case.coords.shape)
    for dtype in (np.float64, np.float32):
        s = case.system(pkg, dtype, coords=x0)
        v0 = s.velocities.copy(); xw = pkg.wrap_coords(s.coords, s.boundary).copy()
        # max_steps = 0: E, and nothing moves
        log4, info = engine_run(pkg, s, 0, 0.1)
        # (fp32: the PME charge spreading adds with float atomics, so two evaluations of one energy differ in their last digits)
        assert info["steps"] == 0 and info["E0"] == info["E"] == pytest.approx(pkg.potential_energy(s), rel=1e-12 if dtype is np.float64 else E_REL[dtype]) and np.array_equal(s.coords, xw)
        # two calls of 6 steps = the host loop called twice (hn starts again)
        t = case.system(pkg, dtype, coords=x0)
        refs = [host_loop(pkg, t, 6, 0.1, init_step=0), host_loop(pkg, t, 6, 0.1, init_step=6)]
        well_separated(dict(E0=refs[0]["E0"], E_trial=refs[0]["E_trial"] + refs[1]["E_trial"], accepted=refs[0]["accepted"] + refs[1]["accepted"]), dtype)
        la, ia = engine_run(pkg, s, 6, 0.1, first=0)
        lb, ib = engine_run(pkg, s, 6, 0.1, first=6)
        assert lb[0, 3] == np.dtype(dtype).type(0.1) and ib["E0"] == pytest.approx(ia["E"], rel=E_REL[dtype])      # (the same coordinates, possibly over another list form)
        agree(slack, f"second of two calls {np.dtype(dtype).name}", dtype, s, lb, ib, refs[1], t.coords, x32=5.9e-6)      # (measured: 2.0e-6)
        assert [bool(a) for a in la[:, 2]] == refs[0]["accepted"]
        assert s.velocities.tobytes() == v0.tobytes()      # bit for bit
        # 20 steps on the same context = the same run on a fresh System built from the pulled state: the held forces were voided
        f = case.system(pkg, dtype, coords=s.coords.copy(), velocities=s.velocities.copy())
        pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 20)
        pkg.simulate(f, pkg.VelocityVerlet(dt=0.0005), 20)
        xb, vb = (1e-9, 1e-7) if dtype is np.float64 else (5e-5, 8e-3)      # (the trajectory bars of tests/test_gpu_pme.py)
        dx = np.asarray(s.coords - f.coords, dtype=np.float64); dx -= case.box * np.round(dx / case.box)
        slack(f"run after a minimisation {np.dtype(dtype).name}: coordinates", np.abs(dx).max(), xb)
        slack(f"run after a minimisation {np.dtype(dtype).name}: velocities", np.abs(s.velocities - f.velocities).max(), vb)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(pkg):
    L = pkg.lib()
    case = S.lj_fluid(8, dtype=np.float64)
    call = lambda s, first=0, n=3, step=0.01, tol=1.0, k=0.0: L.mhip_minimize(s._ctx, first, n, step, tol, k, None, None)
    # before mhip_set_atoms / mhip_set_state
    cfg = pkg.Config(); cfg.precision = 64; cfg.n_atoms = 10; cfg.box[:] = [3.0, 3.0, 3.0]; cfg.periodic[:] = [1, 1, 1]; cfg.r_list = 1.2; cfg.rebuild_every = 10
    cfg.inter.lj_enabled = 1; cfg.inter.lj_cutoff_kind = 1; cfg.inter.lj_rc = 1.0
    ctx = C.c_void_p()
    assert L.mhip_create(C.byref(ctx), C.byref(cfg)) == 0
    try:
        assert L.mhip_minimize(ctx, 0, 3, 0.01, 1.0, 0.0, None, None) == ERR_STATE and b"mhip_minimize" in L.mhip_last_error(ctx)
    finally:
        L.mhip_destroy(ctx)
    # with ghost atoms
    g = case.system(pkg, np.float64); g.push_state()
    assert L.mhip_set_atom_counts(g._ctx, len(g) - 4, 4) == 0
    assert call(g) == ERR_STATE
    # invalid arguments: the context as before
    s = case.system(pkg, np.float64)
    f0, e0 = pkg.forces(s), pkg.potential_energy(s)
    x0 = s.coords.copy()
    for kw in (dict(n=-1), dict(first=-1), dict(step=0.0), dict(step=-0.01), dict(step=np.inf), dict(step=np.nan), dict(tol=np.nan), dict(k=-1.0), dict(k=np.inf), dict(k=np.nan)):
        assert call(s, **kw) == ERR_INVALID, kw
        assert L.mhip_last_error(s._ctx)
    s.pull_state()
    assert np.array_equal(s.coords, x0) and np.array_equal(pkg.forces(s), f0) and pkg.potential_energy(s) == e0
    assert call(s) == 0


# ---- 9. constrained 6mrr ------------------------------------------------------------------------------------------------------------------------
def test_constrained_6mrr_falls_as_the_host_loop_on_the_twin(pkg, slack):
    from molly_jl_amd.workloads import protein_6mrr
    case = protein_6mrr(coulomb="ewald", dtype=np.float32, pme=True, constraints="hbonds", rigid_water=True)
    s = case.system(pkg, np.float32)
    pkg.simulate(s, pkg.SteepestDescentMinimizer(max_steps=50, engine_loop=True))
    assert np.isfinite(s.coords).all()
    t = R.twin_with_bonds(case, 500_000.0).system(pkg, np.float32)
    e0 = pkg.potential_energy(t)
    pkg.simulate(t, pkg.SteepestDescentMinimizer(max_steps=50))
    e_host = pkg.potential_energy(t)
    t.coords[:] = s.coords
    e_engine = pkg.potential_energy(t)
    assert np.isfinite([e0, e_host, e_engine]).all() and e_engine < e0 and e_host < e0
    # the fall of the energy: the two loops end at energies that agree as two fp32 evaluations of one energy do (the project's fp32 potential-energy bar, rel 2e-5;
    # the charge spreading adds with float atomics, so the last digits vary from run to run: measured 0.004 kJ/mol of the 3.4 allowed)
    slack("constrained 6mrr: energy fall, engine loop against host loop [kJ/mol]", abs((e0 - e_engine) - (e0 - e_host)), 2e-5 * abs(e_host))
    print(f"[minimize] constrained 6mrr: E {e0:.1f} → {e_engine:.1f} (host loop {e_host:.1f}); largest |r − d| {R.pair_deviation(case, np.asarray(s.coords, dtype=np.float64)):.3e} nm")
