"""What a rescaling thermostat costs inside mhip_vv_run (fp32): ms/step of 6mrr with PME unconstrained at 0.5 fs, 6mrr with PME, H-bond constraints and rigid
water at 2 fs, and the 256k-atom LJ fluid — each uncoupled, with BerendsenThermostat (applied every step) and with VelocityRescaleThermostat(n_steps = 10), the three
forms alternating over REPEATS rounds in one process (the uncoupled run of the same process is the baseline; the spread over the rounds is printed).  Then the stage
timers of one profiled run of each form: where a coupled step's time goes.
(for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/micro/thermostat_cost.py 1000 1)"""
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
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
SYSTEMS = {
    "6mrr_pme_0.5fs": (lambda: W.protein_6mrr("ewald", T, pme=True), 0.0005, 298.0),
    "6mrr_pme_constrained_2fs": (lambda: W.protein_6mrr("ewald", T, pme=True, constraints="hbonds", rigid_water=True), 0.002, 298.0),
    "lj256k": (lambda: W.lj_fluid(64, seed=2, dtype=T), 0.002, 85.0),
}
COUPLINGS = {
    "uncoupled": lambda temp: None,
    "berendsen_every_step": lambda temp: m.BerendsenThermostat(temp, 0.1),
    "csvr_n_steps_10": lambda temp: m.VelocityRescaleThermostat(temp, 0.1, n_steps=10),
}

for name, (make, dt, temp) in SYSTEMS.items():
    case = make()
    runs = {}
    for form, coupling in COUPLINGS.items():      # one context per form, warmed up: the timed windows alternate between them
        s = case.system(m, T)
        sim = m.VelocityVerlet(dt=dt, coupling=coupling(temp))
        m.simulate(s, sim, 500, rng=1)
        runs[form] = (s, sim, [])
    for r in range(REPEATS):
        for form, (s, sim, ms) in runs.items():
            t = time.perf_counter()
            m.simulate(s, sim, N, init_step=500 + r * N, rng=1)      # returns behind the run's closing synchronisation
            ms.append(1e3 * (time.perf_counter() - t) / N)
    base = min(runs["uncoupled"][2])
    for form, (s, sim, ms) in runs.items():
        n_app = 0 if sim.coupling is None else N // getattr(sim.coupling, "n_steps", 1)
        out = dict(system=name, form=form, ms_per_step=round(min(ms), 5), spread=[round(x, 5) for x in ms], ns_per_day=round(dt * 1e-3 * 86400e3 / min(ms), 1),
                   us_per_application=None if n_app == 0 else round(1e3 * (min(ms) - base) * N / n_app, 2), fused_steps=s.stats()["n_fused_steps"],
                   temperature_K=round(m.temperature(s), 1))
        if sim.coupling is not None:
            out["thermostat_info"] = s.thermostat_info()
        print(out, flush=True)
    for form, coupling in COUPLINGS.items():      # the stage timers, in runs of their own (profiling drains the stream between the stages)
        s = case.system(m, T)
        sim = m.VelocityVerlet(dt=dt, coupling=coupling(temp))
        m.simulate(s, sim, 200, rng=1)
        s._check(m.lib().mhip_set_profiling(s.engine(), 1))
        m.simulate(s, sim, 1000, init_step=200, rng=1)
        st = s.stats()
        print(dict(system=name, form=form, stage_us_per_step=[round(x, 2) for x in st["prof_ms"]], stage_calls=st["prof_calls"]), flush=True)
