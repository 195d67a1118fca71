"""The walk of tests/test_gpu_admit.py and tests/test_gpu_thermostat.py: a feature that runs on a single domain (constraints, virtual sites, a
rescaling thermostat) against every ghosted / domain entry point, in both orders — the feature first, then every entry; a plan first, then the
feature's setter.  Every call returns a status code; after every refusal a 2-step mhip_vv_run must return 0 and leave, bit for bit, the state of a
twin context that made the same calls except the refused one."""
import ctypes as C

import numpy as np

ERR_UNSUPPORTED = -6
DT = 0.002


def empty_plan_and_one_brick(case):
    from molly_jl_amd import _lib
    plan = _lib.HaloPlan()          # no rows, no peers: a valid (empty) plan
    geom = _lib.DomainGeometry()    # one brick, periodic on every axis
    for d in range(3):
        geom.grid[d] = 1; geom.box[d] = float(case.box[d])
    geom.rank = 0; geom.r_ghost = 0.0
    return plan, geom


def walk(pkg, case, turn_on, turn_off, after_run=lambda s, on: None, dtype=np.float64):
    """turn_on(s) / turn_off(s) → status of the feature's setter; after_run(s, on): the caller's own assertions behind every run (made on the twin too); on: the feature is set"""
    L = pkg.lib()
    plan, geom = empty_plan_and_one_brick(case)
    done, reason = C.c_int64(0), C.c_int32(0)
    counters = (C.c_int64 * 8)()

    def fresh():
        s = case.system(pkg, dtype)
        s.push_state(velocities=True)
        return s

    def run_both(s, twin, first, on):
        for c in (s, twin):
            assert L.mhip_vv_run(c._ctx, first, 2, DT, 1) == 0, L.mhip_last_error(c._ctx).decode()
            after_run(c, on)
            c.pull_state()
        assert np.array_equal(s.coords, twin.coords) and np.array_equal(s.velocities, twin.velocities), first

    # (1) the feature is set: every ghosted / domain entry point refuses, and the run goes on after each as if the call had not been made
    s, twin = fresh(), fresh()
    assert turn_on(s) == 0 and turn_on(twin) == 0, L.mhip_last_error(s._ctx).decode()
    step = 0
    for what, call in [
            ("mhip_set_halo_plan", lambda: L.mhip_set_halo_plan(s._ctx, C.byref(plan))),
            ("mhip_set_domain", lambda: L.mhip_set_domain(s._ctx, C.byref(geom), None)),
            ("mhip_halo_region", lambda: L.mhip_halo_region(s._ctx, 64, 2, 0, None)),
            ("mhip_domain_run", lambda: L.mhip_domain_run(s._ctx, step, 2, DT, 0, None, 0, C.byref(done), C.byref(reason), C.cast(counters, C.POINTER(C.c_int64)))),
            ("mhip_vv_halo_start", lambda: L.mhip_vv_halo_start(s._ctx, DT)),
            ("mhip_vv_halo_mid", lambda: L.mhip_vv_halo_mid(s._ctx, step + 1, DT, 0, None, 0)),
            ("mhip_vv_halo_begin", lambda: L.mhip_vv_halo_begin(s._ctx, DT, None, None, 0, None)),
            ("mhip_vv_halo_end", lambda: L.mhip_vv_halo_end(s._ctx, step + 1, DT, 0, 0, None, None)),
            ("mhip_vv_halo_end_parts", lambda: L.mhip_vv_halo_end_parts(s._ctx, step + 1, DT, 0, 0, None, None, 0))]:
        assert call() == ERR_UNSUPPORTED, what
        run_both(s, twin, step, True)
        step += 2
    # (2) a plan is there first: the feature's setter refuses, the context steps without the feature, and takes it once the plan is gone
    for what, set_plan, drop_plan in [
            ("mhip_set_halo_plan", lambda c: L.mhip_set_halo_plan(c._ctx, C.byref(plan)), lambda c: L.mhip_set_halo_plan(c._ctx, None)),
            ("mhip_set_domain", lambda c: L.mhip_set_domain(c._ctx, C.byref(geom), None), lambda c: L.mhip_set_domain(c._ctx, None, None)),
            ("mhip_halo_region", lambda c: L.mhip_halo_region(c._ctx, 64, 2, 0, None), None)]:      # (peers stay: a region is not given back)
        s, twin = fresh(), fresh()
        assert set_plan(s) == 0 and set_plan(twin) == 0, (what, L.mhip_last_error(s._ctx).decode())
        assert turn_on(s) == ERR_UNSUPPORTED, what
        assert turn_off(s) == 0, what      # switching off is always allowed
        run_both(s, twin, 0, False)
        if drop_plan is None:
            continue
        assert drop_plan(s) == 0 and drop_plan(twin) == 0, what
        assert turn_on(s) == 0 and turn_on(twin) == 0, (what, L.mhip_last_error(s._ctx).decode())
        run_both(s, twin, 2, True)
