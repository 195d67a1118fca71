"""6mrr (fp32, PME) with H-bond constraints and rigid water at 2 fs through mhip_vv_run and mhip_langevin_run: ms/step and ns/day over 3000 steps, the
list upkeep and the mhip_constraint_info words; then the same unconstrained at 0.5 fs from the same process.
(for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/micro/constrained_6mrr.py)"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import molly_loader  # noqa: E402

m = molly_loader.load()
W = importlib.import_module("molly_jl_amd.workloads")
T = np.float32
N = int(sys.argv[1]) if len(sys.argv) > 1 else 3000


def run(which, dt, constrained):
    kw = dict(constraints="hbonds", rigid_water=True) if constrained else {}
    s = W.protein_6mrr("ewald", T, pme=True, **kw).system(m, T)
    sim = m.Langevin(dt=dt, temperature=298.0, friction=1.0) if which == "langevin" else m.VelocityVerlet(dt=dt)
    m.simulate(s, sim, 500, rng=1)
    b0 = s.stats()["n_outer_builds"]
    t = time.perf_counter()
    m.simulate(s, sim, N, init_step=500, rng=1)
    el = time.perf_counter() - t
    st = s.stats()
    ms = 1e3 * el / N
    out = dict(run=which, dt_fs=dt * 1e3, constrained=constrained, ms_per_step=round(ms, 5), ns_per_day=round(dt * 1e-3 * 86400e3 / ms, 1),
               outer_builds=st["n_outer_builds"] - b0, fused_steps=st["n_fused_steps"])
    if constrained:
        out["constraint_info"] = s.constraint_info()
        out["temperature_K"] = round(m.temperature(s), 1)
    print(out, flush=True)


for which in ("vv", "langevin"):
    run(which, 0.002, True)
for which in ("vv", "langevin"):
    run(which, 0.0005, False)
