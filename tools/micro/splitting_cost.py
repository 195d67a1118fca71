"""What a LangevinSplitting step costs (fp32, one process): ms/step of "BAOAB", "BAOA" and "BAB" through mhip_splitting_run on the 256k-atom LJ fluid and on 6mrr
with PME, next to mhip_langevin_run (the fused "BAOA") and mhip_vv_run (the fused "BAB") on the same systems, the forms alternating over REPEATS rounds of N steps
(best round, spread printed), with the integrator launches per step of each form.  The yardstick is the only way to run BAOAB without the entry point: the host
loop — one force call and a state round trip per step, the update in numpy — timed the same way over fewer steps.  One JSON line per system and form.
    python tools/micro/splitting_cost.py [N] [REPEATS]"""
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import molly_loader  # noqa: E402

m = molly_loader.load()
W = importlib.import_module("molly_jl_amd.workloads")
from tests import splitting_ref as R  # noqa: E402

T = np.float32
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N_HOST = max(20, N // 20)
KEY = 0x9E3779B97F4A7C15
SYSTEMS = {
    "lj256k": (lambda: W.lj_fluid(64, seed=2, dtype=T), 0.002, 85.0, 1.0),
    "6mrr_pme": (lambda: W.protein_6mrr("ewald", T, pme=True), 0.0005, 298.0, 1.0),
}


def host_baoab(s, n, dt, kT, friction, rng):
    """the host loop: forces from the engine's one-shot call (which takes the coordinates over and hands the forces back), the update in numpy"""
    mass = s.masses.astype(np.float64)[:, None]
    a = friction * dt / mass
    c1, c2 = np.exp(-a), np.sqrt(kT / mass * (1.0 - np.exp(-2.0 * a)))
    x, v = s.coords.astype(np.float64), s.velocities.astype(np.float64)
    f = m.forces(s).astype(np.float64)
    for _ in range(n):
        v += 0.5 * dt * f / mass
        x += 0.5 * dt * v
        v = c1 * v + c2 * rng.normal(size=v.shape)
        x += 0.5 * dt * v
        s.coords[:] = m.wrap_coords(x, s.boundary)
        x = s.coords.astype(np.float64)
        f = m.forces(s).astype(np.float64)
        v += 0.5 * dt * f / mass
        v -= (v * mass).sum(axis=0) / mass.sum()
    s.velocities[:] = v


for name, (make, dt, temp, gamma) in SYSTEMS.items():
    case = make()
    L = m.lib()
    kT = m.BOLTZMANN * temp
    fric = gamma * float(np.mean(case.mass))      # (a mass per time; on the one-mass fluid "BAOA" is then mhip_langevin_run's scheme)
    forms = {
        "splitting_BAOAB": lambda s, first, n: L.mhip_splitting_run(s._ctx, first, n, dt, kT, fric, b"BAOAB", 1, KEY, first),
        "splitting_BAOA": lambda s, first, n: L.mhip_splitting_run(s._ctx, first, n, dt, kT, fric, b"BAOA", 1, KEY, first),
        "splitting_BAB": lambda s, first, n: L.mhip_splitting_run(s._ctx, first, n, dt, kT, fric, b"BAB", 1, KEY, first),
        "langevin_run": lambda s, first, n: L.mhip_langevin_run(s._ctx, first, n, dt, kT, gamma, 1, KEY, first),
        "vv_run": lambda s, first, n: L.mhip_vv_run(s._ctx, first, n, dt, 1),
    }
    runs = {}
    for form, call in forms.items():      # one context per form, warmed up: the timed windows alternate between them
        s = case.system(m, T)
        s.push_state(velocities=True)
        s._check(call(s, 0, 300))
        runs[form] = (s, call, [])
    for r in range(REPEATS):
        for form, (s, call, ms) in runs.items():
            t = time.perf_counter()
            s._check(call(s, 300 + r * N, N))      # returns behind the run's closing synchronisation
            ms.append(1e3 * (time.perf_counter() - t) / N)
    for form, (s, call, ms) in runs.items():
        st = s.stats()
        s.pull_state()
        sp = form.split("_")[1] if form.startswith("splitting") else None
        print(json.dumps(dict(system=name, atoms=case.n, form=form, ms_per_step=round(min(ms), 5), spread=[round(x, 5) for x in ms],
                              segment_launches_per_step=None if sp is None else len(R.plan(sp, dt)["segments"]), fused_steps=st["n_fused_steps"],
                              temperature_K=round(m.temperature(s), 1))), flush=True)
        s.close()
    h = case.system(m, T)
    m.forces(h)
    host_baoab(h, 5, dt, kT, fric, np.random.default_rng(1))
    ms = []
    for r in range(REPEATS):
        t = time.perf_counter()
        host_baoab(h, N_HOST, dt, kT, fric, np.random.default_rng(2 + r))
        ms.append(1e3 * (time.perf_counter() - t) / N_HOST)
    print(json.dumps(dict(system=name, atoms=case.n, form="host_loop_BAOAB", steps=N_HOST, ms_per_step=round(min(ms), 5), spread=[round(x, 5) for x in ms])), flush=True)
