"""SHAKE_RATTLE without a GPU: the 6mrr constraint topology (setup.jl:1576-1630), the clusters and refusals of the numpy reference
(tests/constraints_ref.py), the reference holding its own constraints, the Python mirror's constructors and the C ABI declarations."""
import math
import os

import numpy as np
import pytest

from tests import constraints_ref as R
from tests import systems as S  # noqa: F401  (Case.oracle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sixmrr(**kw):
    import molly_loader
    m = molly_loader.load()
    from importlib import import_module
    return m, import_module("molly_jl_amd.workloads").protein_6mrr(constraints="hbonds", rigid_water=True, **kw)


ref_of = R.of_case


def test_6mrr_hbonds_and_rigid_water_topology():
    m, case = sixmrr()
    c = case.constraints
    assert len(c["dist"]["i"]) == 596 and len(c["angle"]["i"]) == 4928
    cons = ref_of(case)
    sizes = {k: len(v[0]) for k, v in cons.clusters.items()}
    assert sizes == {"2": 186, "3": 133, "4": 48, "angle": 4928}
    assert cons.n_constraints == 15380
    # constrained bonds and angles left the bonded lists: no bond with a hydrogen, no H-O-H angle of a water
    full = __import__("molly_jl_amd.workloads", fromlist=["x"]).protein_6mrr()
    assert len(case.bonds["i"]) == len(full.bonds["i"]) - 596 - 2 * 4928
    assert len(case.angles["i"]) == len(full.angles["i"]) - 4928
    assert not np.any(case.mass[case.bonds["i"]] < 1.1) and not np.any(case.mass[case.bonds["j"]] < 1.1)
    # rigid water alone: the water bonds and angles only, every protein bond stays
    w = __import__("molly_jl_amd.workloads", fromlist=["x"]).protein_6mrr(rigid_water=True)
    assert "dist" not in w.constraints or len(w.constraints["dist"]["i"]) == 0
    assert len(w.constraints["angle"]["i"]) == 4928
    with pytest.raises(ValueError):
        __import__("molly_jl_amd.workloads", fromlist=["x"]).protein_6mrr(constraints="allbonds")


@pytest.mark.parametrize("dist,angle,what", [
    (([0, 1, 2], [1, 2, 3], [0.1] * 3), None, "chain"),
    (([0, 1, 2], [1, 2, 0], [0.1] * 3), None, "ring"),
    (([0, 0, 0, 0], [1, 2, 3, 4], [0.1] * 4), None, "four on one centre"),
    (([0], [1], [0.1]), ([1], [2], [3], [0.1], [0.1], [0.15]), "atom in two clusters"),
    (None, ([0], [1], [2], [0.1], [0.1], [0.2]), "linear angle"),
    (([0], [9], [0.1]), None, "index out of range"),
    (([0], [1], [0.0]), None, "non-positive length"),
])
def test_reference_cluster_refusals(dist, angle, what):
    with pytest.raises(ValueError):
        R.build_clusters(6, dist, angle)


def test_reference_holds_its_own_constraints():
    case = R.toy_system()
    cons = ref_of(case, tol=1e-10)
    o = case.oracle(np.float64)
    x, v = R.vv_run(o, cons, case.coords, case.velocities, 30, 0.002, remove_cm_every=1)
    e_d, e_v = cons.check(x, v)
    assert e_d <= 1e-10 and e_v <= 1e-9, (e_d, e_v)
    x, v = R.langevin_run(o, cons, case.coords, case.velocities, 10, 0.002, 2.494, 1.0, key=5, ctr1=9)
    e_d, _ = cons.check(x, v)
    assert e_d <= 1e-10
    # RATTLE alone: the velocity constraints to rounding
    v2 = v.copy(); cons.rattle(x, v2)
    assert cons.check(x, v2)[1] <= 1e-12


def test_python_mirror_constructors():
    import molly_loader
    m = molly_loader.load()
    a = m.AngleConstraint(0, 1, 2, math.radians(104.52), 0.09572, 0.09572)
    assert abs(a.dist_ik - 2 * 0.09572 * math.sin(math.radians(104.52) / 2)) < 1e-12
    with pytest.raises(ValueError):
        m.AngleConstraint(0, 1, 2, math.pi, 0.1, 0.1)
    sr = m.SHAKE_RATTLE(3, dist_constraints=[m.DistanceConstraint(0, 1, 0.1)], angle_constraints=[a])
    assert sr.n_constraints == 4 and sr.max_iters == 25 and sr.dist_tolerance == 1e-8
    with pytest.raises(ValueError):
        m.SHAKE_RATTLE(3, dist_tolerance=0.0)

    class LINCS:
        pass
    with pytest.raises(m.MollyHipError):
        m.System(coords=np.zeros((3, 3)), boundary=m.CubicBoundary(2.0), constraints=(LINCS(),))
    s = m.System(coords=np.zeros((3, 3)), boundary=m.CubicBoundary(2.0), constraints=(sr,))
    assert s.n_constraints == 4
    # refused before any engine call: the rigid-molecule treatment of the minimiser and the barostat stays in Julia
    with pytest.raises(m.MollyHipError):
        m.virial(s)
    with pytest.raises(m.MollyHipError):
        m.simulate(s, m.SteepestDescentMinimizer())


def test_abi_declares_the_constraint_entry_points():
    h = open(os.path.join(ROOT, "include", "mollyhip.h")).read()
    assert "int32_t mhip_set_constraints(mhip_ctx* ctx, int64_t n_dist" in h and "int32_t mhip_constraint_info(mhip_ctx* ctx, int64_t* out8);" in h
    import molly_loader
    m = molly_loader.load()
    assert "mhip_set_constraints" in m.SIGNATURES and "mhip_constraint_info" in m.SIGNATURES
