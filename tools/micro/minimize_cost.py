"""What a steepest-descent step costs (fp32, 100 steps from a perturbed start, best of three): the engine loop (mhip_minimize) against the host loop of api.py on
6mrr with PME, constrained 6mrr (the host loop runs the twin System that carries the constraints as harmonic bonds: it refuses constraints) and the 256k-atom LJ
fluid, next to the ms per velocity-Verlet step of the same context.  One JSON line per system."""
import copy
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
from tests import minimize_ref as R  # noqa: E402

T = np.float32
N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
K_BOND = 500_000.0


def timed(s, x0, sim):
    ts = []
    for _ in range(3):
        s.coords[:] = x0
        t = time.perf_counter()
        m.simulate(s, sim)
        ts.append(1e3 * (time.perf_counter() - t))
    return ts


def run(name, case, dt, constrained=False):
    x0 = (case.coords + np.random.default_rng(1).normal(scale=0.005, size=case.coords.shape)).astype(T)
    s = case.system(m, T, coords=x0)
    x0 = s.coords.copy()
    m.potential_energy(s)      # context, lists and the PME plan made outside the timed region
    eng = timed(s, x0, m.SteepestDescentMinimizer(max_steps=N, tol=0.0, engine_loop=True, constraint_bond_constant=K_BOND))
    st = s.stats()
    h = (R.twin_with_bonds(case, K_BOND) if constrained else copy.copy(case)).system(m, T, coords=x0)
    m.potential_energy(h)
    host = timed(h, x0, m.SteepestDescentMinimizer(max_steps=N, tol=0.0))
    m.simulate(s, m.VelocityVerlet(dt=dt), 200)      # (from the minimised coordinates)
    t = time.perf_counter()
    m.simulate(s, m.VelocityVerlet(dt=dt), 1000, init_step=200)
    vv = 1e3 * (time.perf_counter() - t) / 1000
    print(json.dumps(dict(system=name, atoms=case.n, steps=N, engine_ms=[round(v, 3) for v in eng], host_ms=[round(v, 3) for v in host],
                          engine_ms_per_step=round(min(eng) / N, 4), host_ms_per_step=round(min(host) / N, 4), vv_ms_per_step=round(vv, 4),
                          faster=bool(max(eng) < min(host)), n_rebuilds=st["n_rebuilds"])), flush=True)


run("6mrr_pme", W.protein_6mrr("ewald", T, pme=True), 0.0005)
run("6mrr_pme_constrained", W.protein_6mrr("ewald", T, pme=True, constraints="hbonds", rigid_water=True), 0.002, constrained=True)
run("lj256k", W.lj_fluid(64, seed=2, dtype=T), 0.002)
