"""mhip_splitting_run and mhip_overdamped_run (csrc/splitting.hip, the loops in csrc/engine.hip) on the MI355X: LangevinSplitting (simulators.jl:1212-1398) and
OverdampedLangevin (:1400-1489) against the numpy restatement of tests/splitting_ref.py over an oracle instance of the same precision, against the existing device loops
where a splitting IS one of them ("BAB", "BAOA"), and the bookkeeping around them: list upkeep, force passes per step, continuation, edges, refusals, sampling.

The bars are the project's own for Langevin runs (tests/test_gpu_stochastic.py): fp64 fluids 1e-9 nm / 1e-7 nm/ps, fp64 6mrr 1e-9 / 1e-6, fp32 against the fp32 oracle
instance 2e-5 / 5e-3 — each tightened to three times the value measured on the MI355X where less than a third of it was used (the rule of `slack`, tests/conftest.py);
the measured value stands beside the bar."""
import ctypes as C

import numpy as np
import pytest

from tests import splitting_ref as R
from tests import systems as S

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -6
KB = 8.314462618e-3
KEY, CTR1 = 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFF0      # (the counter wraps inside every run of more than 16 O sub-steps)
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def split(pkg, s, splitting, n, dt, kT, friction, key=KEY, ctr1=CTR1, first=0, cm=1, push=True, rc=0):
    if push:
        s.push_state(velocities=True)
    got = pkg.lib().mhip_splitting_run(s._ctx, first, n, dt, kT, friction, splitting.encode(), cm, key, ctr1 % 2 ** 64)
    assert got == rc, (got, pkg.lib().mhip_last_error(s._ctx).decode())
    s.pull_state()
    return s


def overdamped(pkg, s, n, dt, kT, gamma, key=KEY, ctr1=CTR1, first=0, cm=1, rc=0):
    s.push_state(velocities=True)
    got = pkg.lib().mhip_overdamped_run(s._ctx, first, n, dt, kT, gamma, cm, key, ctr1 % 2 ** 64)
    assert got == rc, (got, pkg.lib().mhip_last_error(s._ctx).decode())
    s.pull_state()
    return s


def dx_of(a, b, case):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    if case.triclinic is not None:
        bv = np.asarray(case.triclinic["basis"], np.float64).reshape(3, 3)
        return float(np.abs(d - np.round(d @ np.linalg.inv(bv)) @ bv).max())
    return float(np.abs(d - np.round(d / case.box) * case.box).max())


def agree(slack, what, s, o, case, x_bar, v_bar):
    dx, dv = dx_of(s.coords, o.coords, case), float(np.abs(np.asarray(s.velocities, np.float64) - o.vel).max())
    print(f"[splitting] {what}: max |dx| {dx:.3e} nm, max |dv| {dv:.3e} nm/ps")
    slack(what + ": coordinates [nm]", dx, x_bar)
    slack(what + ": velocities [nm/ps]", dv, v_bar)


@pytest.fixture(scope="module")
def charged():
    """1000 atoms of three masses, one of them massless, with exclusions and special pairs"""
    case = S.charged_fluid(10, dict(kind="rf", rc=1.0), dtype=np.float64, with_exceptions=True, stable=True)
    case.mass = np.array(case.mass, np.float64); case.mass[7] = 0.0
    return case


# ---- 1. fp64 parity with the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove_cm", [1, 0])
@pytest.mark.parametrize("splitting", ["BAOAB", "OBABO", "ABOBA", "BAOA", "AOB", "OOA", "BAB"])
def test_fp64_matches_the_restatement(pkg, slack, charged, splitting, remove_cm):
    dt, kT, fric = 0.0005, KB * 300.0, 60.0
    o = charged.oracle(np.float64)
    R.splitting_run(o, 20, dt, kT, fric, splitting, key=KEY, ctr1=CTR1, remove_cm_every=remove_cm, nthreads=4)
    s = split(pkg, charged.system(pkg, np.float64), splitting, 20, dt, kT, fric, cm=remove_cm)
    agree(slack, f"{splitting} cm {remove_cm} fp64", s, o, charged, 2.7e-15, 1.6e-13)      # (measured over the 14 cases: 8.9e-16, 5.2e-14; the project's bars: 1e-9, 1e-7)
    if remove_cm:
        assert np.abs((np.asarray(s.velocities) * charged.mass[:, None]).sum(axis=0)).max() < 1e-9      # remove_CM_motion! after the last step


# ---- 2. fp32 parity: 343 atoms, the second block partial ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitting", ["BAOAB", "OBABO"])
def test_fp32_matches_the_fp32_restatement(pkg, slack, splitting):
    case = S.lj_fluid(7, dtype=np.float32)
    dt, kT, fric = 0.002, KB * 85.0, 1.0 * 39.948
    o = case.oracle(np.float32)
    R.splitting_run(o, 20, dt, kT, fric, splitting, key=KEY, ctr1=CTR1, nthreads=4)
    s = split(pkg, case.system(pkg, np.float32), splitting, 20, dt, kT, fric)
    agree(slack, f"{splitting} fp32", s, o, case, 7.2e-7, 6.1e-7)      # (measured: 2.4e-7, 2.0e-7; the project's bars: 2e-5, 5e-3)


# ---- 3. a small system with side forces: bonded terms + PME, through fold_side_forces -----------------------------------------------------------------
def test_6mrr_pme_fp64_matches_the_restatement(pkg, slack):
    from tests import golden6mrr as G
    case = G.case("ewald", np.float64, bonded=True, pme=True)
    dt, kT, fric = 0.0005, KB * 300.0, 12.0
    o = case.oracle(np.float64)
    R.splitting_run(o, 6, dt, kT, fric, "BAOAB", key=KEY, ctr1=CTR1, nthreads=8, specific=True, general=True)
    s = split(pkg, case.system(pkg, np.float64), "BAOAB", 6, dt, kT, fric)
    agree(slack, "6mrr BAOAB fp64", s, o, case, 4.0e-15, 1.7e-12)      # (measured: 1.3e-15, 5.5e-13; the project's bars: 1e-9, 1e-6)


# ---- 4. against the existing device loops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("andersen", [False, True])
def test_bab_is_mhip_vv_run(pkg, slack, andersen):
    case = S.lj_fluid(8, dtype=np.float64)
    L = pkg.lib()
    a, b = case.system(pkg, np.float64), case.system(pkg, np.float64)
    a.push_state(velocities=True); b.push_state(velocities=True)
    if andersen:
        for s in (a, b):
            assert L.mhip_set_andersen(s._ctx, KB * 120.0, 0.04, 77) == 0
    assert L.mhip_vv_run(a._ctx, 0, 30, 0.002, 1) == 0
    a.pull_state()
    split(pkg, b, "BAB", 30, 0.002, 0.0, 0.0, push=False)
    dx, dv = dx_of(a.coords, b.coords, case), float(np.abs(a.velocities - b.velocities).max())
    print(f"[splitting] BAB against mhip_vv_run (andersen {andersen}): max |dx| {dx:.3e} max |dv| {dv:.3e}")
    slack("BAB against mhip_vv_run: coordinates [nm]", dx, 1.4e-15)      # (measured: 0 and 4.4e-16; the project's bar: 1e-9)
    slack("BAB against mhip_vv_run: velocities [nm/ps]", dv, 2.5e-15)    # (measured: 1.7e-16 and 8.2e-16; 1e-7)
    if andersen:
        plain = case.system(pkg, np.float64); plain.push_state(velocities=True)
        split(pkg, plain, "BAB", 30, 0.002, 0.0, 0.0, push=False)
        assert np.abs(plain.velocities - b.velocities).max() > 0.05      # the coupling really acted


@pytest.mark.parametrize("dtype,n_side,n_steps", [(np.float64, 8, 30), (np.float32, 65, 5)])
def test_baoa_is_mhip_langevin_run(pkg, slack, dtype, n_side, n_steps):
    """… with friction = γ·m on a one-mass fluid; the fp32 case has 274 625 atoms, more than 1 024 blocks' worth: the grid-stride loop"""
    case = S.lj_fluid(n_side, dtype=dtype)
    gamma, dt, kT = 2.0, 0.002, KB * 85.0
    a, b = case.system(pkg, dtype), case.system(pkg, dtype)
    a.push_state(velocities=True)
    assert pkg.lib().mhip_langevin_run(a._ctx, 0, n_steps, dt, kT, gamma, 1, KEY, CTR1) == 0
    a.pull_state()
    split(pkg, b, "BAOA", n_steps, dt, kT, gamma * 39.948)
    dx, dv = dx_of(a.coords, b.coords, case), float(np.abs(np.asarray(a.velocities, np.float64) - b.velocities).max())
    print(f"[splitting] BAOA against mhip_langevin_run {np.dtype(dtype).name}: max |dx| {dx:.3e} max |dv| {dv:.3e}")
    slack("BAOA against mhip_langevin_run: coordinates [nm]", dx, 6.7e-16 if dtype is np.float64 else 5.8e-6)      # (measured: 2.2e-16 | 1.9e-6; the project's bars: 1e-9 | 2e-5)
    slack("BAOA against mhip_langevin_run: velocities [nm/ps]", dv, 1.3e-15 if dtype is np.float64 else 4.3e-6)    # (measured: 4.2e-16 | 1.4e-6; 1e-7 | 5e-3)


# ---- 5. lists across rebuilds ------------------------------------------------------------------------------------------------------------------------------
def test_lists_across_rebuilds(pkg, slack):
    """a hot fluid over six cadence steps: a pair missing from a list for one pass would show as a force jump.  ("BABAB" computes forces twice per step: refused, below)"""
    case = S.lj_fluid(8, temperature=300.0, dtype=np.float64)
    dt, kT, fric = 0.002, KB * 300.0, 80.0
    o = case.oracle(np.float64)
    R.splitting_run(o, 60, dt, kT, fric, "BAOAB", key=KEY, ctr1=CTR1, nthreads=4)
    s = case.system(pkg, np.float64)
    s.push_state(velocities=True)
    r0 = s.stats()["n_rebuilds"]
    split(pkg, s, "BAOAB", 60, dt, kT, fric, push=False)
    st = s.stats()
    print("[splitting] lists: n_rebuilds", r0, "→", st["n_rebuilds"], "filter passes", st["n_filter_passes"])
    assert st["n_rebuilds"] - r0 >= 2
    agree(slack, "BAOAB 60 steps hot fp64", s, o, case, 1.4e-15, 2.1e-14)      # (measured: 4.4e-16, 6.7e-15; the project's bars: 1e-9, 1e-7)
    split(pkg, case.system(pkg, np.float64), "BABAB", 2, dt, kT, fric, rc=ERR_UNSUPPORTED)


# ---- 6. force passes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitting,k", [("BAOAB", 1), ("BAOA", 1), ("AO", 0)])
def test_force_passes_per_step(pkg, splitting, k):
    case = S.lj_fluid(8, dtype=np.float32)
    s = case.system(pkg, np.float32)
    s.push_state(velocities=True)
    n = 23
    c0 = s.stats()["n_force_calls"]
    split(pkg, s, splitting, n, 0.002, KB * 85.0, 40.0, push=False)
    c1 = s.stats()["n_force_calls"]
    split(pkg, s, splitting, n, 0.002, KB * 85.0, 40.0, first=n, ctr1=CTR1 + n, push=False)
    c2 = s.stats()["n_force_calls"]
    print(f"[splitting] {splitting}: force passes {c1 - c0} then {c2 - c1} over {n} steps")
    assert n * k <= c1 - c0 <= n * k + 1 and n * k <= c2 - c1 <= n * k + 1
    if k == 0:
        assert c2 == c0      # no pass at all


# ---- 7. continuation ----------------------------------------------------------------------------------------------------------------------------------------
def test_continuation_reproducibility_and_keys(pkg, slack):
    case = S.lj_fluid(8, dtype=np.float64)
    dt, kT, fric, sp = 0.002, KB * 85.0, 80.0, "OBABO"      # two O per step
    whole = split(pkg, case.system(pkg, np.float64), sp, 25, dt, kT, fric)
    cut = case.system(pkg, np.float64)
    split(pkg, cut, sp, 10, dt, kT, fric)
    split(pkg, cut, sp, 15, dt, kT, fric, first=10, ctr1=CTR1 + 10 * 2, push=False)
    # (measured: 0 and 0 — the second call takes the first one's last forces and keeps its lists; the project's bars are 1e-9 and 1e-7, three units in the last place stand here)
    slack("10 + 15 against 25: coordinates [nm]", dx_of(whole.coords, cut.coords, case), 1.4e-15)
    slack("10 + 15 against 25: velocities [nm/ps]", np.abs(whole.velocities - cut.velocities).max(), 3.4e-16)
    again = split(pkg, case.system(pkg, np.float64), sp, 25, dt, kT, fric)
    assert np.array_equal(whole.coords, again.coords) and np.array_equal(whole.velocities, again.velocities)
    other = split(pkg, case.system(pkg, np.float64), sp, 25, dt, kT, fric, key=KEY + 1)
    assert np.abs(whole.velocities - other.velocities).max() > 1e-3


# ---- 8. edges --------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_atom_two_atoms_and_the_longest_string(pkg, slack):
    one = S.Case([[1.0, 1.0, 1.0]], 4.0, lj=dict(cutoff=("distance", 1.0)), r_list=1.2, velocities=[[0.3, -0.2, 0.1]], sigma=[0.3], eps=[0.5], mass=[10.0])
    two = S.Case([[0.2, 2.0, 2.0], [3.85, 2.0, 2.0]], 4.0, lj=dict(cutoff=("distance", 1.0)), r_list=1.2, velocities=[[0.2, 0.1, 0.0], [-0.3, 0.0, 0.1]],
                 sigma=[0.3, 0.32], eps=[0.5, 0.4], mass=[10.0, 12.0])      # a pair across the periodic face
    for case in (one, two):
        o = case.oracle(np.float64)
        R.splitting_run(o, 12, 0.002, KB * 300.0, 30.0, "BAOAB", key=KEY, ctr1=CTR1, remove_cm_every=0)
        s = split(pkg, case.system(pkg, np.float64), "BAOAB", 12, 0.002, KB * 300.0, 30.0, cm=0)
        agree(slack, f"{case.n} atom(s) BAOAB fp64", s, o, case, 1.4e-15, 2.5e-15)      # (measured: 0, 8.3e-16; the project's bars: 1e-9, 1e-7; coordinates: three units in the last place)
    sixteen = "BAOOOOOOOOOOOOAB"      # 16 sub-steps, twelve counters per step, one force computation
    o = two.oracle(np.float64)
    R.splitting_run(o, 3, 0.002, KB * 300.0, 30.0, sixteen, key=KEY, ctr1=CTR1, remove_cm_every=1)
    s = split(pkg, two.system(pkg, np.float64), sixteen, 3, 0.002, KB * 300.0, 30.0)
    agree(slack, "16 sub-steps fp64", s, o, two, 1.4e-15, 5.0e-16)      # (measured: 0, 1.7e-16)
    split(pkg, two.system(pkg, np.float64), sixteen + "A", 3, 0.002, KB * 300.0, 30.0, rc=ERR_INVALID)


def test_triclinic_matches_the_restatement(pkg, slack):
    from tests.test_gpu_triclinic import sheared_fluid
    basis, case = sheared_fluid(np.float64)
    dt, kT, fric = 0.002, KB * 120.0, 80.0
    o = case.oracle(np.float64)
    R.splitting_run(o, 8, dt, kT, fric, "BAOAB", key=KEY, ctr1=CTR1, nthreads=8)
    s = split(pkg, case.system(pkg, np.float64), "BAOAB", 8, dt, kT, fric)
    agree(slack, "triclinic BAOAB fp64", s, o, case, 5.4e-15, 1.2e-13)      # (measured: 1.8e-15, 3.9e-14; the project's bars: 1e-9, 1e-7)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(pkg):
    from tests.test_gpu_virtual_sites import set_sites
    L = pkg.lib()
    case = S.lj_fluid(8, dtype=np.float64)
    i32 = lambda *a: np.array(a, np.int32)
    f64 = lambda *a: np.array(a, np.float64)
    both = lambda s, **kw: (L.mhip_splitting_run(s._ctx, kw.get("first", 0), kw.get("n", 3), kw.get("dt", 0.002), kw.get("kT", 2.0), kw.get("fric", 5.0),
                                                 kw.get("sp", b"BAOAB"), 1, 1, 2),
                            L.mhip_overdamped_run(s._ctx, kw.get("first", 0), kw.get("n", 3), kw.get("dt", 0.002), kw.get("kT", 2.0), kw.get("fric", 5.0), 1, 1, 2))

    def fresh(mass0=None):
        c = case
        if mass0 is not None:
            c = S.lj_fluid(8, dtype=np.float64); c.mass = c.mass.copy(); c.mass[mass0] = 0.0
        s = c.system(pkg, np.float64)
        s.push_state(velocities=True)
        return s

    def unchanged(s, f0):
        assert np.array_equal(pkg.forces(s), f0)

    s = fresh(); f0 = pkg.forces(s)
    # constraints, virtual sites
    assert L.mhip_set_constraints(s._ctx, 1, p(i32(0)), p(i32(1)), p(f64(0.36)), 0, None, None, None, None, 1e-8, 1e-8, 25) == 0
    assert both(s) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and b"constraints" in L.mhip_last_error(s._ctx)
    assert L.mhip_set_constraints(s._ctx, 0, None, None, None, 0, None, None, None, None, 1e-8, 1e-8, 25) == 0
    unchanged(s, f0)
    v = fresh(mass0=3); fv = pkg.forces(v)
    assert set_sites(L, v, [(1, 3, 0, -1, -1, 0, 0, 0, 0, 0, 0)]) == 0
    assert both(v) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and b"virtual sites" in L.mhip_last_error(v._ctx)
    assert L.mhip_set_virtual_sites(v._ctx, 0, None, None, None, None, None, None) == 0
    unchanged(v, fv)
    # a rescaling thermostat
    assert L.mhip_set_thermostat(s._ctx, 2, KB * 120.0, 0.1, 1, 3 * len(s) - 3, 0, 0) == 0
    assert both(s) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and b"mhip_overdamped_run" in L.mhip_last_error(s._ctx)
    assert L.mhip_set_thermostat(s._ctx, 0, 0.0, 0.0, 1, 0, 0, 0) == 0
    unchanged(s, f0)
    # ghosts
    g = fresh()
    assert L.mhip_set_atom_counts(g._ctx, len(g) - 4, 4) == 0
    assert both(g) == (ERR_STATE, ERR_STATE)
    # arguments
    for kw in (dict(n=-1), dict(first=-1), dict(dt=np.inf), dict(dt=np.nan), dict(kT=-1.0), dict(fric=-1.0)):
        assert both(s, **kw) == (ERR_INVALID, ERR_INVALID), kw
        unchanged(s, f0)
    for sp in (b"", b"BAoAB", b"BAXAB", b"BAOAB ", b"BAOABBAOABBAOABBA", None):
        assert L.mhip_splitting_run(s._ctx, 0, 3, 0.002, 2.0, 5.0, sp, 1, 1, 2) == ERR_INVALID and b"splitting" in L.mhip_last_error(s._ctx), sp
        unchanged(s, f0)
    for fric in (0.0, np.inf, np.nan):
        assert both(s, fric=fric)[1] == ERR_INVALID, fric      # γ must be positive and finite
    assert both(s, fric=0.0)[0] == 0                           # … while a splitting takes friction 0
    assert both(s, n=0) == (0, 0)
    assert both(s) == (0, 0)                                   # … and the context runs
    # the Python mirror
    with pytest.raises(pkg.MollyHipError):
        pkg.simulate(fresh(), pkg.LangevinSplitting(0.002, 85.0, 40.0, "BAOAB", coupling=pkg.ImmediateThermostat(85.0)), 2)
    with pytest.raises(pkg.MollyHipError):
        pkg.simulate(fresh(), pkg.LangevinSplitting(0.002, 85.0, 40.0, "BAOAB", coupling=pkg.MonteCarloBarostat(1.0, 85.0, fresh().boundary)), 2)


def test_simulate_draws_key_then_counter(pkg):
    """the Python mirror: key, then ctr1 (simulators.jl:1291-1292); a splitting without an O draws nothing; AndersenThermostat couples"""
    case = S.lj_fluid(8, dtype=np.float64)
    rng = np.random.default_rng(21)
    key, ctr1 = (int(rng.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(2))
    a = case.system(pkg, np.float64)
    pkg.simulate(a, pkg.LangevinSplitting(dt=0.002, temperature=85.0, friction=40.0, splitting="BAOAB"), 10, rng=21)
    b = split(pkg, case.system(pkg, np.float64), "BAOAB", 10, 0.002, KB * 85.0, 40.0, key=key, ctr1=ctr1)
    assert np.array_equal(a.coords, b.coords) and np.array_equal(a.velocities, b.velocities)
    g = np.random.default_rng(5); state = g.bit_generator.state
    pkg.simulate(case.system(pkg, np.float64), pkg.LangevinSplitting(dt=0.002, temperature=85.0, friction=40.0, splitting="BAB"), 3, rng=g)
    assert g.bit_generator.state == state
    c = case.system(pkg, np.float64)
    pkg.simulate(c, pkg.LangevinSplitting(0.002, 85.0, 40.0, "BAB", coupling=pkg.AndersenThermostat(300.0, 0.02)), 10, rng=3)
    d = case.system(pkg, np.float64)
    pkg.simulate(d, pkg.VelocityVerlet(dt=0.002, coupling=pkg.AndersenThermostat(300.0, 0.02)), 10, rng=3)
    assert np.abs(c.velocities - d.velocities).max() < 1e-7 and np.abs(c.velocities - a.velocities).max() > 0.05
    e = case.system(pkg, np.float64)
    pkg.simulate(e, pkg.OverdampedLangevin(dt=0.0005, temperature=85.0, friction=50.0), 5, rng=21)
    f = overdamped(pkg, case.system(pkg, np.float64), 5, 0.0005, KB * 85.0, 50.0, key=key, ctr1=ctr1)
    assert np.array_equal(e.coords, f.coords)


# ---- 10. sampling --------------------------------------------------------------------------------------------------------------------------------------------
def test_baoab_thermalises_the_lj_fluid(pkg):
    """85 K argon driven to 140 K.  The instantaneous temperature of 4 096 atoms scatters by T·sqrt(2/(3N)) = 1.8 K: the bar of 5.6 K is above three standard
    deviations even if the ten samples were fully correlated (the bar of test_langevin_thermalises_the_lj_fluid)"""
    case = S.lj_fluid(16, dtype=np.float32)
    s = case.system(pkg, np.float32)
    sim = pkg.LangevinSplitting(dt=0.002, temperature=140.0, friction=5.0 * 39.948, splitting="BAOAB")
    pkg.simulate(s, sim, 1000, rng=1)
    ts = []
    for k in range(10):
        pkg.simulate(s, sim, 50, init_step=1000 + 50 * k, rng=100 + k)
        ts.append(pkg.temperature(s))
    print("[splitting] BAOAB at 140 K: mean T", np.mean(ts))
    assert abs(np.mean(ts) - 140.0) < 0.04 * 140.0
    assert np.isfinite(s.coords).all()


# ---- 11. overdamped ----------------------------------------------------------------------------------------------------------------------------------------------
def test_overdamped_fp64_matches_the_restatement(pkg, slack, charged):
    """γ = 1000/ps: the Euler–Maruyama step of this fluid is stable only where dt·k/(m·γ) stays well below 2 for its stiffest contact and its 1 u atoms.  At 50/ps the
    restatement ALONE turns a 1e-14 nm change of one coordinate into 2.1e-4 nm within the 20 steps (and the device run then differs from it by 5.7e-4 nm); at 1000/ps
    the same change ends at 9.9e-15 nm, and two correct implementations can be compared at round-off"""
    dt, kT, gamma = 0.0005, KB * 300.0, 1000.0
    o = charged.oracle(np.float64)
    v0 = o.vel.copy()
    R.overdamped_run(o, 20, dt, kT, gamma, key=KEY, ctr1=CTR1, nthreads=4)
    s0 = charged.system(pkg, np.float64)
    s = overdamped(pkg, charged.system(pkg, np.float64), 20, dt, kT, gamma)
    agree(slack, "overdamped fp64", s, o, charged, 1.4e-15, 1.7e-16)      # (measured: 4.4e-16, 5.6e-17 — one ulp each; the project's bars: 1e-9, 1e-7)
    assert np.array_equal(s.coords[7], pkg.wrap_coords(s0.coords, s0.boundary)[7])      # the massless atom stays
    vc = (v0 * charged.mass[:, None]).sum(axis=0) / charged.mass.sum()
    assert np.abs(s.velocities - (v0 - vc)).max() < 1e-12                               # remove_CM_motion!, nothing else
    assert np.abs(np.asarray(s.coords) - s0.coords).max() > 1e-3


def test_overdamped_fp32_matches_the_fp32_restatement(pkg, slack):
    case = S.lj_fluid(7, dtype=np.float32)
    dt, kT, gamma = 0.0005, KB * 85.0, 50.0
    o = case.oracle(np.float32)
    R.overdamped_run(o, 20, dt, kT, gamma, key=KEY, ctr1=CTR1, nthreads=4)
    s = overdamped(pkg, case.system(pkg, np.float32), 20, dt, kT, gamma)
    agree(slack, "overdamped fp32", s, o, case, 7.2e-7, 5.6e-9)      # (measured: 6.0e-8 in one run and 2.4e-7, one ulp of a coordinate above 2 nm, in another; 1.9e-9 — the velocities see remove_CM_motion! alone; the project's bars: 2e-5, 5e-3)
