"""What admit.h's table refuses, through the C ABI on the device: constraints and virtual sites against every ghosted / domain entry point, in both
call orders (tests/admit_walk.py; the rescaling thermostats take the same walk in tests/test_gpu_thermostat.py).  The closing kick of
mhip_vv_halo_end / mhip_vv_halo_end_parts has no RATTLE and spreads no site force: both refuse; mhip_set_halo_plan and mhip_halo_region with peers
refuse the two features as mhip_set_domain does, and the features' setters refuse a halo plan as they refuse a domain plan.  The context steps on,
bit for bit, after every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import admit_walk
from tests import systems as S
from tests import virtual_sites_ref as V

pytestmark = pytest.mark.gpu

p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def fluid257(site=None):
    """the first 257 atoms of a one-type fluid (two blocks, ragged); site: that atom massless and without a Lennard-Jones well"""
    full = S.lj_fluid(7, seed=3, dtype=np.float32)
    n = 257
    mass, eps = full.mass[:n].copy(), full.eps[:n].copy()
    if site is not None:
        mass[site] = 0.0; eps[site] = 0.0
    return S.Case(full.coords[:n], full.box, lj=full.lj, r_list=full.r_list, rebuild_every=full.rebuild_every, velocities=full.velocities[:n],
                  sigma=full.sigma[:n], eps=eps, mass=mass, name="lj_first257" + ("" if site is None else "_site"))


def test_constraints_against_halo_and_domain_plans(pkg):
    """one distance constraint on atoms 0 and 1, at the distance they start at"""
    L = pkg.lib()
    case = fluid257()
    d = np.asarray(case.coords[1], np.float64) - np.asarray(case.coords[0], np.float64)
    d -= np.asarray(case.box, np.float64) * np.round(d / np.asarray(case.box, np.float64))
    i, j, r0 = np.array([0], np.int32), np.array([1], np.int32), np.array([np.linalg.norm(d)], np.float64)
    on = lambda s: L.mhip_set_constraints(s._ctx, 1, p(i), p(j), p(r0), 0, None, None, None, None, 1e-8, 1e-8, 25)
    off = lambda s: L.mhip_set_constraints(s._ctx, 0, None, None, None, 0, None, None, None, None, 1e-8, 1e-8, 25)
    admit_walk.walk(pkg, case, on, off)


def test_virtual_sites_against_halo_and_domain_plans(pkg):
    """one two-parent site (atom 2, halfway between atoms 0 and 1) on a massless atom"""
    L = pkg.lib()
    case = fluid257(site=2)
    t, a, a1, a2, a3, w = V.site_arrays([(2, 2, 0, 1, -1, 0.5, 0.5, 0, 0, 0, 0)])
    on = lambda s: L.mhip_set_virtual_sites(s._ctx, len(t), p(t), p(a), p(a1), p(a2), p(a3), p(w))
    off = lambda s: L.mhip_set_virtual_sites(s._ctx, 0, None, None, None, None, None, None)
    admit_walk.walk(pkg, case, on, off)
