"""What voids what the context holds (molly.jl_amd/csrc/held.h), seen from outside: a run of 7 steps, ONE change made to the live context straight
through the C ABI, the run continued for 5 steps with init_step=7 — against a fresh context started from the same (x7, v7) with the change in place
from its start.  The continued run must not use anything the change voided (the forces the first leg left, lists without the new exclusion, a check
measured for the old velocities), and may keep everything else: in fp64 the two end within 1e-9 nm and 1e-7 nm/ps of each other (the bars of
test_gpu_cadence.py::test_terms_added_between_two_runs_count_from_the_first_step, which covers the bonded setters in the same way; rounding alone
separates the two, the continued run walking lists in another order).  Sizes: those of the cadence tests."""
import ctypes as C

import numpy as np
import pytest

from tests import systems as S

pytestmark = pytest.mark.gpu

X_BAR, V_BAR = 1e-9, 1e-7      # nm, nm/ps
MEM_HOST = 0


def _restart(case, x, v, **over):
    """the case again from (x, v), with some of its fields replaced"""
    f = dict(lj=case.lj, coul=case.coul, r_list=case.r_list, rebuild_every=case.rebuild_every, charge=case.charge, sigma=case.sigma, eps=case.eps,
             mass=case.mass, excluded=case.excluded, special=case.special, pme=case.pme)
    f.update(over)
    return S.Case(x, case.box, velocities=v, **f)


def _close(a, b):
    dx, dv = np.abs(a.coords - b.coords).max(), np.abs(a.velocities - b.velocities).max()
    print(f"max |dx| {dx:.3e} nm (bar {X_BAR:g}), max |dv| {dv:.3e} nm/ps (bar {V_BAR:g})")
    assert dx < X_BAR and dv < V_BAR, (dx, dv)


def _first_leg(pkg, case, dt):
    sim = pkg.VelocityVerlet(dt=dt, remove_CM_motion=0)
    a = case.system(pkg, np.float64)
    pkg.simulate(a, sim, 7)
    assert a.stats()["n_filter_passes"] > 0, a.stats()      # the dual list is in use: an outer list and an inner one pruned from it
    return sim, a, a.coords.copy(), a.velocities.copy()


def _push_atoms_only(pkg, a):
    a._check(pkg.lib().mhip_set_atoms(a.engine(), a._ptr(a.charge), a._ptr(a.σ), a._ptr(a.ϵ), a._ptr(a.masses), a._ptr(a.λ), MEM_HOST))


def test_charges_changed_between_two_runs(pkg):
    """mhip_set_atoms with other charges: the lists stand (same atoms, same places), the forces of the first leg's last step do not"""
    case = S.charged_fluid(14, dict(kind="rf", rc=1.0), dtype=np.float64, stable=True)
    sim, a, x7, v7 = _first_leg(pkg, case, 0.0005)
    q = case.charge * np.where(np.arange(case.n) % 2 == 0, 0.8, 1.1)
    a.charge = np.ascontiguousarray(q)      # (a new array: the System may share the case's)
    _push_atoms_only(pkg, a)
    pkg.simulate(a, sim, 5, init_step=7)
    b = _restart(case, x7, v7, charge=q).system(pkg, np.float64)
    pkg.simulate(b, sim, 5, init_step=7)
    _close(a, b)
    c = _restart(case, x7, v7).system(pkg, np.float64)      # (with the old charges the legs end elsewhere)
    pkg.simulate(c, sim, 5, init_step=7)
    assert np.abs(a.velocities - c.velocities).max() > 100 * V_BAR


def test_exclusion_added_between_two_runs(pkg):
    """mhip_set_exceptions with more excluded pairs: every list is void, for the pairs are taken out when the lists are made"""
    case = S.charged_fluid(14, dict(kind="rf", rc=1.0), dtype=np.float64, stable=True)
    sim, a, x7, v7 = _first_leg(pkg, case, 0.0005)
    outer7 = a.stats()["n_outer_builds"]
    more = np.array([[i, i + 1] for i in range(2, 200, 3)])      # lattice neighbours 0.31 nm apart that were neither excluded (i % 3 == 0) nor special
    excluded = np.vstack([case.excluded, more])
    ex = np.ascontiguousarray(excluded, dtype=np.int32); sp = np.ascontiguousarray(case.special, dtype=np.int32)
    exi, exj, spi, spj = (np.ascontiguousarray(c) for c in (ex[:, 0], ex[:, 1], sp[:, 0], sp[:, 1]))
    a.neighbor_finder.excluded = ex
    a._check(pkg.lib().mhip_set_exceptions(a.engine(), a._ptr(exi), a._ptr(exj), len(exi), a._ptr(spi), a._ptr(spj), len(spi)))
    pkg.simulate(a, sim, 5, init_step=7)
    b = _restart(case, x7, v7, excluded=excluded).system(pkg, np.float64)
    pkg.simulate(b, sim, 5, init_step=7)
    _close(a, b)
    assert a.stats()["n_outer_builds"] > outer7, a.stats()      # searched again
    # the new exclusions matter at these bars: the same legs without them end elsewhere
    c = _restart(case, x7, v7).system(pkg, np.float64)
    pkg.simulate(c, sim, 5, init_step=7)
    assert np.abs(a.coords - c.coords).max() > 100 * X_BAR


def test_pme_switched_on_between_two_runs(pkg):
    """mhip_set_pme on a context that ran with the direct-space part alone: the first step of the second leg carries the reciprocal-space forces"""
    case = S.charged_fluid(14, dict(kind="ewald", rc=1.0), dtype=np.float64, stable=True, with_exceptions=False)
    sim, a, x7, v7 = _first_leg(pkg, case, 0.0005)
    b = _restart(case, x7, v7, pme=dict(order=5)).system(pkg, np.float64)
    gi = b.general_inters[0]
    a.general_inters = (gi,)
    a._check(pkg.lib().mhip_set_pme(a.engine(), gi.order, (C.c_int32 * 3)(*gi.mesh_dims), gi.α, gi.ϵr))
    pkg.simulate(a, sim, 5, init_step=7)
    pkg.simulate(b, sim, 5, init_step=7)
    _close(a, b)
    c = _restart(case, x7, v7).system(pkg, np.float64)      # (without the mesh part the legs end elsewhere)
    pkg.simulate(c, sim, 5, init_step=7)
    assert np.abs(a.velocities - c.velocities).max() > 100 * V_BAR


def test_velocities_alone_replaced_between_two_runs(pkg):
    """mhip_set_state with velocities and no coordinates: the forces of the coordinates stand, the lists are looked at again for the new speeds"""
    case = S.lj_fluid(10, dtype=np.float64)
    sim, a, x7, v7 = _first_leg(pkg, case, 0.002)
    v_new = -1.5 * v7[::-1]      # other speeds, other directions, no net momentum
    a.velocities[:] = v_new
    a._check(pkg.lib().mhip_set_state(a.engine(), None, a._ptr(a.velocities), MEM_HOST))
    pkg.simulate(a, sim, 5, init_step=7)
    b = _restart(case, x7, v_new).system(pkg, np.float64)
    pkg.simulate(b, sim, 5, init_step=7)
    _close(a, b)
    assert np.abs(a.coords - x7).max() > 1e-3      # (the second leg moved with the new speeds)


@pytest.mark.parametrize("side", [10, 12])
def test_same_state_handed_back_redoes_nothing(pkg, side):
    """the state the engine holds, handed back unchanged (what every continued simulate does): the lists, the forces of the last step and the check in
    flight all stand — the two legs search, prune and launch exactly as often as one run of 12 steps, and end where a fresh start from (x7, v7) ends"""
    case = S.lj_fluid(side, dtype=np.float64)
    sim, a, x7, v7 = _first_leg(pkg, case, 0.002)
    pkg.simulate(a, sim, 5, init_step=7)
    st = a.stats()
    b = _restart(case, x7, v7).system(pkg, np.float64)
    pkg.simulate(b, sim, 5, init_step=7)
    _close(a, b)
    u = case.system(pkg, np.float64)
    pkg.simulate(u, sim, 12)
    su = u.stats()
    for k in ("n_outer_builds", "n_filter_passes", "n_force_calls"):
        assert st[k] == su[k], (k, st[k], su[k])
    assert np.array_equal(a.coords, u.coords) and np.array_equal(a.velocities, u.velocities)      # same lists, same order, same forces: the same bits
