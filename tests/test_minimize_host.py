"""The steepest-descent loop restated in numpy (tests/minimize_ref.py) on closed forms, and the host side of mhip_minimize: the header's declaration against
the ctypes signature, the dataclass's defaults, the refusals the default path keeps, and the engine path's own error without a device."""
import os
import re

import numpy as np
import pytest

from tests import minimize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_harmonic_well_sequence_can_be_written_down():
    """E = k/2 |x|², one atom at distance a: every trial moves it by hn along −x (F/‖F‖ is the unit vector), so the step is accepted exactly while
    |a − hn| < a, i.e. hn < 2a — the whole accept / reject / hn sequence follows from a and step_size alone"""
    k, a, h0, n = 3.0, 1.0, 0.5, 14
    out = R.loop(np.array([[a, 0.0, 0.0]]), lambda x: -k * x, lambda x: 0.5 * k * float((x * x).sum()), h0, n, tol=0.0)
    r, hn, want, hs = a, h0, [], []
    for _ in range(n):
        hs.append(hn)
        if abs(r - hn) < r:
            r = abs(r - hn); hn = 6 * hn / 5; want.append(True)
        else:
            hn = hn / 5; want.append(False)
    assert out["accepted"] == want and True in want and False in want
    assert out["hn_used"] == pytest.approx(hs, rel=1e-14) and out["hn"] == pytest.approx(hn, rel=1e-14)
    assert abs(out["coords"][0, 0]) == pytest.approx(r, abs=1e-14) and out["E"] == pytest.approx(0.5 * k * r * r, rel=1e-12)
    assert out["max_force"][0] == pytest.approx(k * a)


def test_lj_dimer_converges_to_the_minimum():
    sigma, eps = 0.3, 0.8

    def energy(x):
        r = np.linalg.norm(x[1] - x[0]); s6 = (sigma / r) ** 6
        return 4 * eps * (s6 * s6 - s6)

    def force(x):
        d = x[1] - x[0]; r = np.linalg.norm(d); s6 = (sigma / r) ** 6
        f = 24 * eps * (2 * s6 * s6 - s6) / r * d / r
        return np.array([-f, f])
    out = R.loop(np.array([[0.0, 0.0, 0.0], [0.42, 0.0, 0.0]]), force, energy, 0.05, 400, tol=1e-6)
    r = np.linalg.norm(out["coords"][1] - out["coords"][0])
    assert r == pytest.approx(2 ** (1 / 6) * sigma, abs=1e-7) and out["E"] == pytest.approx(-eps, abs=1e-9)
    assert True in out["accepted"] and False in out["accepted"] and out["max_force"][-1] < 1e-6


def test_zero_force_stops_without_the_division():
    out = R.loop(np.array([[0.3, 0.2, 0.1]]), lambda x: np.zeros_like(x), lambda x: 0.0, 0.01, 5, tol=1.0)
    assert out["accepted"] == [False] and np.array_equal(out["coords"], [[0.3, 0.2, 0.1]])


def test_twin_with_bonds_carries_every_constrained_pair(pkg):
    from tests import constraints_ref
    case = constraints_ref.toy_system(2)
    i, j, d = R.constrained_pairs(case)
    c = case.constraints
    assert len(i) == len(c["dist"]["i"]) + 3 * len(c["angle"]["i"]) and (d > 0).all()
    t = R.twin_with_bonds(case, 5e5)
    assert t.constraints is None and case.constraints is not None and len(t.bonds["i"]) == len(i) and set(t.bonds["k"]) == {5e5}
    assert np.array_equal(t.excluded, case.excluded)
    assert R.twin_with_bonds(case, None).bonds is None
    assert R.pair_deviation(case, case.coords) < 1e-12


def test_header_declares_mhip_minimize_and_the_signature_has_it(pkg):
    import ctypes as C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mollyhip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+mhip_minimize\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/mollyhip.h does not declare mhip_minimize"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mhip_ctx* ctx", "int64_t first_step", "int64_t max_steps", "double step_size", "double tol", "double constraint_bond_k", "double* log4", "double* out8"]
    res, args = pkg.SIGNATURES["mhip_minimize"]
    assert res is C.c_int32 and args[:6] == [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double] and len(args) == 8
    assert pkg.lib().mhip_minimize(None, 0, 1, 0.01, 1.0, 0.0, None, None) == -1      # null context
    abi = open(os.path.join(ROOT, "julia", "ext", "mhip_abi.jl")).read()
    assert "(:mhip_minimize, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64})" in abi


def test_dataclass_defaults(pkg):
    sim = pkg.SteepestDescentMinimizer()
    assert (sim.step_size, sim.max_steps, sim.tol, sim.log_stream, sim.constraint_bond_constant, sim.engine_loop) == (0.01, 1000, 1000.0, None, 500_000.0, False)
    assert pkg.SteepestDescentMinimizer(0.02, 5, 1.0, None, None, True).constraint_bond_constant is None      # the two new fields trail the old ones


def _constrained(pkg):
    sr = pkg.SHAKE_RATTLE(3, dist_constraints=[pkg.DistanceConstraint(0, 1, 0.1)])
    return pkg.System(coords=np.array([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [1.2, 1.2, 1.2]]), boundary=pkg.CubicBoundary(2.0), pairwise_inters=(pkg.LennardJones(),), constraints=(sr,))


def _with_site(pkg):
    x = np.array([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [1.2, 1.2, 1.2], [0.55, 0.5, 0.5]])
    return pkg.System(coords=x, boundary=pkg.CubicBoundary(2.0), pairwise_inters=(pkg.LennardJones(),), virtual_sites=(pkg.TwoParticleAverageSite(3, 0, 1, 0.5, 0.5),),
                      mass=np.array([1.0, 1.0, 1.0, 0.0]))


def test_default_path_still_refuses_constraints_and_sites(pkg):
    for s in (_constrained(pkg), _with_site(pkg)):
        with pytest.raises(pkg.MollyHipError) as e:
            pkg.simulate(s, pkg.SteepestDescentMinimizer())
        assert e.value.code == -6


def test_engine_loop_without_a_device_is_the_no_device_error(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible")
    for s in (_constrained(pkg), _with_site(pkg)):
        with pytest.raises(pkg.MollyHipError) as e:
            pkg.simulate(s, pkg.SteepestDescentMinimizer(engine_loop=True, max_steps=2))
        assert e.value.code == -5      # MHIP_ERR_NO_DEVICE, not a refusal
    with pytest.raises(ValueError):
        pkg.simulate(_constrained(pkg), pkg.SteepestDescentMinimizer(engine_loop=True), init_step=-1)
