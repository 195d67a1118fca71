"""The rescaling thermostats (ImmediateThermostat, BerendsenThermostat, VelocityRescaleThermostat; csrc/thermostat.h, thermostat_step.h,
mhip_set_thermostat) inside the device velocity-Verlet loop, through the C ABI, against the fp64 numpy restatement of tests/thermostat_ref.py:
the reduction's edges, trajectory parity on every route of the step loop, the identities between the kinds, chunked continuation bit for
bit, the launch accounting, every refusal, and once the physics (constrained 6mrr at 2 fs held at 300 K)."""
import ctypes as C

import numpy as np
import pytest

from tests import constraints_ref as CR
from tests import golden6mrr as G
from tests import systems as S
from tests import thermostat_ref as TR
from tests import virtual_sites_ref as V

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -6
KB = TR.KB
KEY, CTR1 = 0x1234567890ABCDEF, 0x0FEDCBA987654321


def truncated(case, n):
    """the first n atoms of a one-type fluid, in its box"""
    return S.Case(case.coords[:n], case.box, lj=case.lj, r_list=case.r_list, rebuild_every=case.rebuild_every, velocities=case.velocities[:n],
                  sigma=case.sigma[:n], eps=case.eps[:n], mass=case.mass[:n], name=f"{case.name}_first{n}")


def dof_of(s):
    return 3 * (len(s) - len(s.virtual_sites)) - 3 - s.n_constraints


def min_image(d, box):
    return d - box * np.round(d / box)


def dev(a, b, box):
    return float(np.abs(min_image(np.asarray(a, np.float64) - np.asarray(b, np.float64), box)).max())


def info_of(pkg, s):
    out = (C.c_double * 8)()
    assert pkg.lib().mhip_thermostat_info(s._ctx, out) == 0
    return list(out)


def raw_run(pkg, case, dtype, runs, dt, cm, thermo=None, profiling=False):
    """runs: (first, n) chunks of mhip_vv_run; thermo: the arguments of mhip_set_thermostat behind the context → System (state pulled), info record"""
    L = pkg.lib()
    s = case.system(pkg, dtype)
    s.push_state(velocities=True)
    if profiling:
        assert L.mhip_set_profiling(s._ctx, 1) == 0
    if thermo is not None:
        assert L.mhip_set_thermostat(s._ctx, *thermo) == 0, L.mhip_last_error(s._ctx).decode()
    for first, n in runs:
        assert L.mhip_vv_run(s._ctx, first, n, dt, cm) == 0, L.mhip_last_error(s._ctx).decode()
    s.pull_state()
    return s, info_of(pkg, s)


def abi_args(th):
    return (th.kind, th.kT, th.coupling_const, th.n_steps, th.dof, th.key, th.ctr1)


# ---- reduction edges -------------------------------------------------------------------------------------------------------------------
_fluids = {}


def fluid(n):
    """2 atoms, 257 (two blocks, ragged), 70 000 (above 256 x 256 lanes: k_vv_open and the close launch loop per lane)"""
    if n not in _fluids:
        side = {2: 7, 257: 7, 70000: 42}[n]
        _fluids[n] = truncated(S.lj_fluid(side, seed=3, dtype=np.float32), n)
    return _fluids[n]


_edge_ref = {}


def edge_reference(n, cm):
    """the fp64 reference chain of 3 Immediate steps, computed once per (n, cm)"""
    if (n, cm) not in _edge_ref:
        case = fluid(n)
        th = TR.Thermostat(TR.IMMEDIATE, 120.0, 3 * n - 3)
        o = case.oracle(np.float64)
        _edge_ref[(n, cm)] = TR.run(TR.oracle_step(o, 0.002, cm, nthreads=8), case.coords, case.velocities, case.mass, 3, 0.002, th)
    return _edge_ref[(n, cm)]


@pytest.mark.parametrize("cm", [1, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 257, 70000])
def test_immediate_reaches_the_target_at_the_reduction_edges(pkg, slack, n, dtype, cm):
    case = fluid(n)
    th = TR.Thermostat(TR.IMMEDIATE, 120.0, 3 * n - 3)
    s, info = raw_run(pkg, case, dtype, [(0, 3)], 0.002, cm, abi_args(th))
    assert dof_of(s) == th.dof and info[0] == 3 and info[1] == 3 and info[6] == 0
    # fp32: one rounding of λ to T (6e-8 relative, twice in the energy) plus the rounding of every velocity, summed
    slack("temperature(sys) against the target (relative)", abs(pkg.temperature(s) - 120.0) / 120.0, 1e-12 if dtype == np.float64 else 2e-6)
    _, _, log = edge_reference(n, cm)
    step, K, lam, _, _ = log[-1]
    # the engine's chain against the fp64 reference's: in fp64 they differ by summation order over three steps; in fp32 by the rounding of the
    # velocities the sums are taken over (6e-8 each) and of three steps of fp32 forces (4e-5 of a kick that is ~1 % of a velocity)
    bar = 1e-10 if dtype == np.float64 else 2e-5
    slack("info: K of the last application (relative)", abs(info[3] - K) / K, bar)
    slack("info: λ of the last application (relative)", abs(info[2] - lam) / lam, bar)
    assert min(info[4], info[5]) <= info[2] <= max(info[4], info[5])


# ---- trajectory parity, fp64, every kind, every route --------------------------------------------------------------------------------------
_routes = {}
CON_TOL = 1e-13


def route(name):
    """→ dict(case, step(dt, cm) → one uncoupled reference step, m, box, dt, cm, n): the four routes of the step loop"""
    if name in _routes:
        return _routes[name]
    if name == "plain":            # k_vv_mid / k_vv_open
        case = truncated(S.lj_fluid(7, seed=3, dtype=np.float64), 257)
        o = case.oracle(np.float64)
        r = dict(case=case, step=TR.oracle_step(o, 0.002, 1), dt=0.002, cm=1, n=20, randn3=o.randn3)
    elif name == "small":          # bonded terms + PME: the side force array, k_gather_collect_vv on the uncoupled steps
        case = G.case("ewald", np.float64, bonded=True, pme=True)
        o = case.oracle(np.float64)
        r = dict(case=case, step=TR.oracle_step(o, 0.0005, 1, nthreads=8, specific=True, general=True), dt=0.0005, cm=1, n=5, randn3=o.randn3)
    elif name == "constrained_1e-10":      # k_con_step at the tolerance the other constraint tests run at
        case = CR.toy_system()
        case.constraints = dict(case.constraints, dist_tolerance=1e-10, max_iters=25)
        o = case.oracle(np.float64)
        cons = CR.of_case(case, tol=1e-10)
        r = dict(case=case, step=TR.constrained_step(o, cons, 0.002, 5), dt=0.002, cm=5, n=20, randn3=o.randn3, cons=cons)
    elif name == "constrained":    # k_con_step
        case = CR.toy_system()
        # SHAKE is iterative: at a tolerance of 1e-10 nm the reference's solve and the engine's stop up to 1e-10 nm apart, which would be what the
        # comparison measures.  1e-13 nm puts the solver below the effect under test (the order of summation, ~1e-15 a step).
        case.constraints = dict(case.constraints, dist_tolerance=CON_TOL, max_iters=100)
        o = case.oracle(np.float64)
        cons = CR.of_case(case, tol=CON_TOL)
        r = dict(case=case, step=TR.constrained_step(o, cons, 0.002, 5), dt=0.002, cm=5, n=20, randn3=o.randn3, cons=cons)
    else:                          # hosted virtual sites: rigid four-site water at 2 fs
        case = V.tip4p_box(8, rigid=True)
        case.constraints = dict(case.constraints, dist_tolerance=1e-10, max_iters=25)
        o = case.oracle(np.float64)
        cons = CR.of_case(case, tol=1e-10)
        r = dict(case=case, step=TR.sites_step(V.oracle_forces(o), cons, case.virtual_sites, case.mass, case.box, 0.002, 1), dt=0.002, cm=1, n=20,
                 randn3=o.randn3, cons=cons)
    _routes[name] = r
    return r


def thermostat_of(kind, r, dof, n_steps=1):
    return {"off": None,
            "immediate": TR.Thermostat(TR.IMMEDIATE, 300.0, dof),
            "berendsen": TR.Thermostat(TR.BERENDSEN, 300.0, dof, coupling_const=0.1),
            "csvr": TR.Thermostat(TR.CSVR, 300.0, dof, coupling_const=0.1, n_steps=n_steps, key=KEY, ctr1=CTR1, randn3=r["randn3"])}[kind]


def parity(pkg, name, kind, n_steps=1):
    """(coordinate deviation [nm], velocity deviation [nm/ps], System, engine info, reference log) of one route under one coupling"""
    r = route(name)
    case = r["case"]
    s0 = case.system(pkg, np.float64)
    th = thermostat_of(kind, r, dof_of(s0), n_steps)
    s, info = raw_run(pkg, case, np.float64, [(0, r["n"])], r["dt"], r["cm"], None if th is None else abi_args(th))
    key = (name, kind, n_steps)
    if key not in _parity_ref:
        _parity_ref[key] = TR.run(r["step"], case.coords, case.velocities, case.mass, r["n"], r["dt"], th)
    x, v, log = _parity_ref[key]
    return dev(s.coords, x, case.box), float(np.abs(s.velocities - v).max()), s, info, log


_parity_ref = {}

# The bars: for each route the same comparison with the coupling OFF on the library of the commit before the thermostats, times 3 (the
# margin the virtual-site tests use for the same reason: the order of summation differs between the reference and the engine).
# Measured on an MI355X, coupling off (coords nm, velocities nm/ps, RATTLE's v_ij·r_ij/|r_ij| nm/ps); DESIGN §10e has both columns.
UNCOUPLED = {"plain": (2.220446049250313e-16, 7.494005416219807e-16, 0.0),
             "small": (3.552713678800501e-15, 1.3717915692268434e-12, 0.0),
             "constrained": (1.4371837053772651e-13, 3.6914915568786455e-12, 8.326672684688676e-16),
             "sites": (1.199040866595169e-14, 7.50871587129609e-13, 1.1000289430881051e-15)}


@pytest.mark.parametrize("kind,n_steps", [("immediate", 1), ("berendsen", 1), ("csvr", 1), ("csvr", 4)])
@pytest.mark.parametrize("name", ["plain", "small", "constrained", "sites"])
def test_trajectory_matches_the_reference(pkg, slack, name, kind, n_steps):
    dx, dv, s, info, log = parity(pkg, name, kind, n_steps)
    assert info[0] == len(log) and info[1] == log[-1][0] and info[6] == 0
    bx, bv, be = UNCOUPLED[name]
    slack("coords vs numpy reference (nm)", dx, 3 * bx)
    slack("velocities vs numpy reference (nm/ps)", dv, 3 * bv)
    slack("info: λ of the last application against the reference chain (relative)", abs(info[2] - log[-1][2]) / log[-1][2], 1e-9)
    r = route(name)
    if "cons" in r:      # a uniform scale commutes with RATTLE: the constraints hold as the uncoupled run leaves them (test_gpu_constraints, test_gpu_virtual_sites)
        e_d, e_v = r["cons"].check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
        slack("constraint lengths (nm)", e_d, r["case"].constraints["dist_tolerance"])
        slack("v_ij . r_ij / |r_ij| (nm/ps)", e_v, 3 * be)            # the level the uncoupled run leaves it at


@pytest.mark.parametrize("kind,n_steps", [("immediate", 1), ("berendsen", 1), ("csvr", 1), ("csvr", 4)])
def test_constrained_trajectory_at_the_production_tolerance(pkg, slack, kind, n_steps):
    """The k_con_thermo launches against the reference with SHAKE at dist_tolerance = 1e-10 nm, the setting of test_gpu_constraints.  Two iterative
    solves that each stop within the tolerance of the constraint surface may stop up to that tolerance apart, and differently so under every coupling
    (uncoupled on the library before the thermostats: 1.6e-11 nm; a multiple of THAT figure is a multiple of where two solvers happened to stop, which is
    why the 3x bars above are taken at 1e-13).  What can be held here is the solver's own bound: coordinates within dist_tolerance, velocities within
    dist_tolerance / dt (SHAKE's correction v += Δx / dt carries the same difference)."""
    name = "constrained_1e-10"
    dx, dv, s, info, log = parity(pkg, name, kind, n_steps)
    r = route(name)
    tol = r["case"].constraints["dist_tolerance"]
    assert info[0] == len(log) and info[1] == log[-1][0] and info[6] == 0
    slack("coords vs numpy reference (nm)", dx, tol)
    slack("velocities vs numpy reference (nm/ps)", dv, tol / r["dt"])
    slack("info: λ of the last application against the reference chain (relative)", abs(info[2] - log[-1][2]) / log[-1][2], 1e-9)
    e_d, e_v = r["cons"].check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
    slack("constraint lengths (nm)", e_d, tol)
    slack("v_ij . r_ij / |r_ij| (nm/ps)", e_v, 3 * 7.257994315992016e-16)      # 3x the uncoupled run at this tolerance on the library before the thermostats


# ---- identities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "constrained"])
def test_berendsen_with_tau_equal_dt_is_immediate(pkg, slack, name):
    r = route(name)
    case = r["case"]
    dof = dof_of(case.system(pkg, np.float64))
    a, _ = raw_run(pkg, case, np.float64, [(0, 20)], r["dt"], r["cm"], (TR.IMMEDIATE, KB * 300.0, 1.0, 1, dof, 0, 0))
    b, _ = raw_run(pkg, case, np.float64, [(0, 20)], r["dt"], r["cm"], (TR.BERENDSEN, KB * 300.0, r["dt"], 1, dof, 0, 0))
    slack("coords, Berendsen(τ = dt) against Immediate (nm)", dev(a.coords, b.coords, case.box), 1e-13)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["plain", "constrained"])
def test_csvr_with_tiny_tau_lands_on_the_drawn_energy(pkg, slack, name, dtype):
    """τ = 1e-9 ps: c = 0, so every application leaves K = ½ kT (R² + S) whatever K was"""
    r = route(name)
    case = r["case"]
    L = pkg.lib()
    s = case.system(pkg, dtype)
    s.push_state(velocities=True)
    dof = dof_of(s)
    o = case.oracle(dtype)
    th = TR.Thermostat(TR.CSVR, 300.0, dof, coupling_const=1e-9, key=KEY, ctr1=CTR1, randn3=o.randn3)      # (the normals of the precision under test)
    assert L.mhip_set_thermostat(s._ctx, *abi_args(th)) == 0
    worst = 0.0
    for step in range(1, 5):      # cut after every application: the kinetic energy of the moment is the thermostat's
        assert L.mhip_vv_run(s._ctx, step - 1, 1, r["dt"], 0) == 0
        ke = C.c_double(0)
        assert L.mhip_kinetic_energy(s._ctx, C.byref(ke)) == 0
        R, Sx = TR.noise(th, step, len(s))
        want = 0.5 * th.kT * (R * R + Sx)
        worst = max(worst, abs(ke.value - want) / want)
    slack("K after an application against ½kT(R² + S) (relative)", worst, 1e-12 if dtype == np.float64 else 2e-6)


# ---- chunking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["plain", "constrained"])
def test_chunked_runs_continue_bit_for_bit(pkg, name, dtype):
    r = route(name)
    case = r["case"]
    dof = dof_of(case.system(pkg, dtype))
    th = (TR.CSVR, KB * 300.0, 0.1, 4, dof, KEY, CTR1)
    one, i1 = raw_run(pkg, case, dtype, [(0, 20)], r["dt"], 0, th)
    assert i1[0] == 5 and i1[1] == 20
    for runs in ([(0, 8), (8, 12)], [(0, 7), (7, 13)]):      # the cut on an application step (8) and between two applications (7)
        two, i2 = raw_run(pkg, case, dtype, runs, r["dt"], 0, th)
        assert np.array_equal(one.coords, two.coords) and np.array_equal(one.velocities, two.velocities), runs
        assert i2[:7] == i1[:7]
    th1 = (TR.BERENDSEN, KB * 300.0, 0.1, 1, dof, 0, 0)      # every step an application: any cut is on one
    one, _ = raw_run(pkg, case, dtype, [(0, 20)], r["dt"], 0, th1)
    two, _ = raw_run(pkg, case, dtype, [(0, 7), (7, 13)], r["dt"], 0, th1)
    assert np.array_equal(one.coords, two.coords) and np.array_equal(one.velocities, two.velocities)


# ---- launch accounting ------------------------------------------------------------------------------------------------------------------
def test_launch_accounting_and_kind_0_restores_the_context(pkg):
    case = S.lj_fluid(16, seed=2, dtype=np.float32)      # 4 096 atoms, one type, fp32
    L = pkg.lib()
    off, _ = raw_run(pkg, case, np.float32, [(0, 100)], 0.002, 1, profiling=True)
    st_off = off.stats()
    th = (TR.CSVR, KB * 85.0, 0.1, 10, 3 * case.n - 3, KEY, CTR1)
    on, info = raw_run(pkg, case, np.float32, [(0, 100)], 0.002, 1, th, profiling=True)
    st_on = on.stats()
    n_app = 10
    print(f"uncoupled: n_fused_steps {st_off['n_fused_steps']}, prof_calls[2] {st_off['prof_calls'][2]}; coupled: {st_on['n_fused_steps']}, {st_on['prof_calls'][2]}")
    assert info[0] == n_app and info[1] == 100
    assert st_on["n_fused_steps"] >= st_off["n_fused_steps"] - n_app
    assert st_on["prof_calls"][2] == st_off["prof_calls"][2] + n_app
    # kind 0 afterwards: the uncoupled run again, bit for bit, with the same fused steps
    ref, _ = raw_run(pkg, case, np.float32, [(0, 100)], 0.002, 1)
    s = case.system(pkg, np.float32)
    s.push_state(velocities=True)
    assert L.mhip_set_thermostat(s._ctx, *th) == 0
    assert L.mhip_set_thermostat(s._ctx, 0, 0.0, 0.0, 1, 0, 0, 0) == 0
    assert L.mhip_vv_run(s._ctx, 0, 100, 0.002, 1) == 0
    s.pull_state()
    assert np.array_equal(s.coords, ref.coords) and np.array_equal(s.velocities, ref.velocities)
    assert s.stats()["n_fused_steps"] == ref.stats()["n_fused_steps"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    L = pkg.lib()
    case = fluid(257)

    def fresh():
        s = case.system(pkg, np.float64)
        s.push_state(velocities=True)
        return s
    ok = (TR.BERENDSEN, KB * 120.0, 0.1, 1, 3 * 257 - 3, 0, 0)
    s = fresh()
    for bad in [(4,) + ok[1:], (-1,) + ok[1:], (2, 0.0) + ok[2:], (2, -1.0) + ok[2:], (2, ok[1], 0.0) + ok[3:], (2, ok[1], 0.1, 0) + ok[4:],
                (1, ok[1], 0.1, 2) + ok[4:], (2, ok[1], 0.1, 3) + ok[4:]]:
        assert L.mhip_set_thermostat(s._ctx, *bad) == ERR_INVALID, bad
    assert L.mhip_set_thermostat(s._ctx, 3, ok[1], 0.1, 3, ok[4], 1, 2) == 0      # VelocityRescale takes n_steps
    assert L.mhip_thermostat_info(s._ctx, None) == ERR_INVALID
    # the Andersen coupling, either order
    assert L.mhip_set_andersen(s._ctx, 2.494, 0.1, 3) == ERR_UNSUPPORTED
    assert L.mhip_set_thermostat(s._ctx, 0, 0.0, 0.0, 1, 0, 0, 0) == 0
    assert L.mhip_set_andersen(s._ctx, 2.494, 0.1, 3) == 0
    assert L.mhip_set_thermostat(s._ctx, *ok) == ERR_UNSUPPORTED
    assert L.mhip_set_andersen(s._ctx, 0.0, 0.0, 0) == 0
    assert L.mhip_set_thermostat(s._ctx, *ok) == 0
    # the split step, the Langevin run, ghosts
    assert L.mhip_vv_init(s._ctx, 0) == 0
    assert L.mhip_vv_stage1(s._ctx, 0.002) == ERR_UNSUPPORTED
    assert L.mhip_vv_stage2(s._ctx, 1, 0.002) == ERR_UNSUPPORTED
    assert L.mhip_langevin_run(s._ctx, 0, 2, 0.002, 2.494, 1.0, 1, 11, 12) == ERR_UNSUPPORTED
    assert L.mhip_set_atom_counts(s._ctx, 253, 4) == ERR_UNSUPPORTED
    # … and the context is still usable: the coupled run, then the Langevin run once the thermostat is unset
    assert L.mhip_vv_run(s._ctx, 0, 3, 0.002, 1) == 0
    assert info_of(pkg, s)[0] == 3
    assert L.mhip_set_thermostat(s._ctx, 0, 0.0, 0.0, 1, 0, 0, 0) == 0
    assert L.mhip_langevin_run(s._ctx, 3, 2, 0.002, 2.494, 1.0, 1, 11, 12) == 0
    # a context with ghosts refuses the thermostat
    s2 = fresh()
    assert L.mhip_set_atom_counts(s2._ctx, 253, 4) == 0
    assert L.mhip_set_thermostat(s2._ctx, *ok) == ERR_UNSUPPORTED
    # the Python mirror: not a coupling of Langevin, not next to AndersenThermostat
    s3 = case.system(pkg, np.float32)
    with pytest.raises(pkg.MollyHipError):
        pkg.simulate(s3, pkg.Langevin(dt=0.002, temperature=120.0, friction=1.0, coupling=pkg.BerendsenThermostat(120.0, 0.1)), 2)
    with pytest.raises(pkg.MollyHipError):
        pkg.simulate(s3, pkg.VelocityVerlet(dt=0.002, coupling=(pkg.AndersenThermostat(120.0, 0.1), pkg.ImmediateThermostat(120.0))), 2)
    pkg.simulate(s3, pkg.VelocityVerlet(dt=0.002, coupling=pkg.ImmediateThermostat(120.0)), 3)
    assert abs(pkg.temperature(s3) - 120.0) < 120.0 * 2e-6 and s3.thermostat_info()["n_applied"] == 3
    pkg.simulate(s3, pkg.VelocityVerlet(dt=0.002), 3, init_step=3)      # unset in simulate's finally: an uncoupled run follows
    assert s3.thermostat_info()["n_applied"] == 3


def test_refusals_with_halo_and_domain_plans(pkg):
    """the halo entry points, mhip_set_halo_plan, mhip_set_domain, mhip_halo_region with peers and mhip_domain_run refuse a context with a thermostat set;
    mhip_set_thermostat refuses a context that has a halo plan, a domain plan or peers; the context is usable after every refusal (tests/admit_walk.py)"""
    from tests import admit_walk
    L = pkg.lib()
    ok = (TR.BERENDSEN, KB * 120.0, 0.1, 1, 3 * 257 - 3, 0, 0)
    off = (0, 0.0, 0.0, 1, 0, 0, 0)

    def after_run(s, on):
        if on:      # (simulate-style: the record counts the applications of the run just made)
            assert info_of(pkg, s)[0] == 2
            assert L.mhip_set_thermostat(s._ctx, *ok) == 0      # "since set": the record starts again
    admit_walk.walk(pkg, fluid(257), lambda s: L.mhip_set_thermostat(s._ctx, *ok), lambda s: L.mhip_set_thermostat(s._ctx, *off), after_run)


# ---- physics, once ----------------------------------------------------------------------------------------------------------------------
def test_constrained_6mrr_at_2fs_is_held_at_300K(pkg, slack):
    """H-bond constraints + rigid water, PME, fp32, velocity Verlet at 2 fs with VelocityRescaleThermostat(300 K, 0.1 ps).  The uncoupled run
    heats to ≈ 395 K when SHAKE snaps the flexible start onto the constraints; 500 steps (10 τ) are skipped, then the mean temperature
    of 250 steps must lie within 4·T₀·sqrt(2/dof) of 300 K — the canonical spread of the INSTANTANEOUS temperature, a generous bound on a mean."""
    from molly_jl_amd.workloads import protein_6mrr
    case = protein_6mrr(coulomb="ewald", dtype=np.float32, pme=True, constraints="hbonds", rigid_water=True)
    s = case.system(pkg, np.float32)
    sim = pkg.VelocityVerlet(dt=0.002, coupling=pkg.VelocityRescaleThermostat(300.0, 0.1))
    pkg.simulate(s, sim, 500, rng=5)
    dof = dof_of(s)
    L = pkg.lib()
    assert L.mhip_set_thermostat(s._ctx, TR.CSVR, KB * 300.0, 0.1, 1, dof, KEY, CTR1) == 0
    temps = []
    for step in range(500, 750):
        assert L.mhip_vv_run(s._ctx, step, 1, 0.002, 1) == 0
        ke = C.c_double(0)
        assert L.mhip_kinetic_energy(s._ctx, C.byref(ke)) == 0
        temps.append(2 * ke.value / (dof * KB))
    assert L.mhip_set_thermostat(s._ctx, 0, 0.0, 0.0, 1, 0, 0, 0) == 0
    print(f"dof {dof}, mean T {np.mean(temps):.2f} K, std {np.std(temps):.2f} K, canonical {300.0 * np.sqrt(2.0 / dof):.2f} K")
    slack("| mean temperature − 300 K | (K)", abs(float(np.mean(temps)) - 300.0), 4 * 300.0 * np.sqrt(2.0 / dof))
    assert s.constraint_info()["n_not_converged"] == 0
    # the fp32 bars of the uncoupled 1000-step run (test_gpu_constraints): a uniform scale leaves the constraints where RATTLE put them
    s.pull_state()
    e_d, e_v = CR.of_case(case, tol=1e-8).check(s.coords.astype(np.float64), s.velocities.astype(np.float64))
    slack("constraint lengths after 750 coupled steps (nm)", e_d, 1e-5)
    slack("v_ij . r_ij / |r_ij| after 750 coupled steps (nm/ps)", e_v, 3.5e-5)


def test_fp32_four_site_water_coupled_holds_the_uncoupled_bars(pkg, slack):
    """rigid TIP4P-FB with PME, fp32, 2 fs, Berendsen every step: the sites stay on place(parents) and the constraints hold at the bars of the
    uncoupled 1000-step run (test_gpu_virtual_sites.test_fp32_pme_1000_steps)"""
    case = V.tip4p_box(12, coulomb="pme")
    cons = CR.of_case(case, tol=1e-8)
    s = case.system(pkg, np.float32)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002, coupling=pkg.BerendsenThermostat(300.0, 0.1)), 200)
    info = s.thermostat_info()
    assert info["n_applied"] == 200 and info["n_refused"] == 0 and s.constraint_info()["n_not_converged"] == 0
    xs = s.coords.astype(np.float64)
    slack("sites on place(parents) (nm)", dev(xs, V.place(xs, case.box, case.virtual_sites), case.box), 4 * 1.2e-7)
    e_d, _ = cons.check(xs, s.velocities.astype(np.float64))
    slack("constraint lengths (nm)", e_d, 1e-5)
