"""Rigid four-site water (TIP4P-FB, tests/golden/tip4p_fb.json) through mhip_vv_run and mhip_langevin_run, fp32, PME, 2 fs: ms/step of (a) the four-site box —
the site M hosted by its water's work item of k_con_step — and (b) the same box with M removed and its charge on O (three sites, constraints only), in one
process, plus the integrator stage's launches per step (prof_calls[2]) from a short profiled run of each.
    python tools/micro/tip4p_water.py [n_side=16] [steps=3000]         (16³ = 4 096 waters, 16 384 atoms)
(for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/micro/tip4p_water.py 16 300)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import molly_loader  # noqa: E402

m = molly_loader.load()
from tests import virtual_sites_ref as V  # noqa: E402  (the box generator is the tests')

T = np.float32
N_SIDE = int(sys.argv[1]) if len(sys.argv) > 1 else 16
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3000


def run(which, three_site):
    case = V.tip4p_box(N_SIDE, rigid=True, coulomb="pme", three_site=three_site)
    s = case.system(m, T)
    sim = m.Langevin(dt=0.002, temperature=300.0, friction=1.0) if which == "langevin" else m.VelocityVerlet(dt=0.002)
    m.simulate(s, sim, 500, rng=1)
    t = time.perf_counter()
    m.simulate(s, sim, N, init_step=500, rng=1)
    el = time.perf_counter() - t
    ms = 1e3 * el / N
    # a short profiled run of its own: the stage timers serialise the stream, so it is not the one that is timed
    L = m.lib()
    s._check(L.mhip_set_profiling(s.engine(), 1))
    st0 = s.stats()
    m.simulate(s, sim, 200, init_step=500 + N, rng=1)
    st1 = s.stats()
    calls = (st1["prof_calls"][2] - st0["prof_calls"][2]) / 200.0
    names = ("pair", "search", "integrator", "sort", "prune_pass", "bonded", "pme")      # the stage timers of mhip_stats
    stage_us = {k: round(1e3 * (st1["prof_ms"][i] - st0["prof_ms"][i]) / 200.0, 2) for i, k in enumerate(names)}
    s._check(L.mhip_set_profiling(s.engine(), 0))
    out = dict(run=which, sites=3 if three_site else 4, atoms=case.n, waters=N_SIDE ** 3, ms_per_step=round(ms, 5), ns_per_day=round(0.002e-3 * 86400e3 / ms, 1),
               integrator_launches_per_step=round(calls, 3), stage_us_per_step=stage_us, constraint_info=s.constraint_info(), temperature_K=round(m.temperature(s), 1))
    if not three_site:
        out["virtual_site_info"] = s.virtual_site_info()
    print(json.dumps(out), flush=True)
    return ms, stage_us


for which in ("vv", "langevin"):
    (a, sa), (b, sb) = run(which, False), run(which, True)
    print(json.dumps(dict(run=which, four_minus_three_site_us_per_step=round(1e3 * (a - b), 2), by_stage_us={k: round(sa[k] - sb[k], 2) for k in sa})), flush=True)
