"""fp64 numpy restatement of the reference's rescaling thermostats (coupling.jl:86-91 ImmediateThermostat, :124-168
VelocityRescaleThermostat, :232-238 BerendsenThermostat) as the coupling of simulate!(sys, VelocityVerlet) (simulators.jl:627-643: the
centre-of-mass removal first, the coupling behind it).  It drives the existing references ONE STEP AT A TIME — the oracle's vv_run,
constraints_ref.vv_run, virtual_sites_ref.vv_run with n_steps = 1 — and applies the coupling between the steps.  The noise of
VelocityRescaleThermostat is OracleSystem.randn3: application at step s uses (key, ctr1 + s); atom i owns its three normals, numbered
k = 3i + c; R is k = 0 and S the sum of the squares of 1 <= k <= dof − 1 (the reference's own sum of dof − 1 squared normals)."""
from dataclasses import dataclass

import numpy as np

KB = 8.314462618e-3
IMMEDIATE, BERENDSEN, CSVR = 1, 2, 3
EPS = float(np.finfo(np.float64).eps)


@dataclass
class Thermostat:
    kind: int
    temperature: float
    dof: int
    coupling_const: float = 1.0
    n_steps: int = 1
    key: int = 0
    ctr1: int = 0
    randn3: object = None       # randn3(i, key, ctr1) → three normals of atom i (CSVR only)

    @property
    def kT(self):
        return KB * self.temperature


def kinetic_energy(v, m):
    v = np.asarray(v, np.float64); m = np.asarray(m, np.float64)
    return 0.5 * float((m[:, None] * v * v).sum())


def noise(th, step, n_atoms):
    """(R, S) of the application at `step`"""
    k_last = th.dof - 1
    n_i = min(n_atoms, k_last // 3 + 1)
    z = np.array([th.randn3(i, th.key, (th.ctr1 + step) % 2 ** 64) for i in range(n_i)], np.float64).reshape(-1)
    return float(z[0]), float((z[1:k_last + 1] ** 2).sum())


def scale(th, K, dt, R=0.0, S=0.0):
    """λ of one application; dof <= 0 or K <= 0: 1 (the reference returns early for VelocityRescale; stated deviation for the other two)"""
    if th.dof <= 0 or not K > 0:
        return 1.0
    temp = 2 * K / (th.dof * KB)
    if th.kind == IMMEDIATE:
        return float(np.sqrt(th.temperature / temp))
    if th.kind == BERENDSEN:
        lam2 = 1 + (dt / th.coupling_const) * (th.temperature / temp - 1)
        return float(np.sqrt(lam2)) if lam2 >= 0 else 1.0
    Kbar = th.dof * KB * th.temperature / 2
    c = np.exp(-(dt * th.n_steps) / th.coupling_const)
    A = Kbar / (th.dof * K)
    lam2 = c + (1 - c) * A * (R * R + S) + 2 * np.sqrt(c * (1 - c) * A) * R
    return float(np.sqrt(max(lam2, EPS)))


def run(step_fn, x, v, m, n_steps, dt, th, first_step=0):
    """step_fn(x, v, first_step) → (x, v) after ONE uncoupled step (its CM removal included).  Returns x, v and the record of every
    application: (step, K before scaling, λ, R, S)."""
    log = []
    for step in range(first_step + 1, first_step + n_steps + 1):
        x, v = step_fn(x, v, step - 1)
        v = np.array(v, np.float64)
        if th is not None and step % th.n_steps == 0:
            K = kinetic_energy(v, m)
            R, S = noise(th, step, len(m)) if th.kind == CSVR else (0.0, 0.0)
            lam = scale(th, K, dt, R, S)
            v = lam * v
            log.append((step, K, lam, R, S))
    return x, v, log


# ---- one uncoupled step of each existing reference ---------------------------------------------------------------------------------------
def oracle_step(o, dt, remove_cm_every, **force_kw):
    """the oracle's vv_run (plain, bonded and PME systems); o: an fp64 OracleSystem"""
    def step(x, v, first):
        o.coords[:] = x; o.vel[:] = v
        o.vv_run(1, dt, first_step=first, remove_cm_every=remove_cm_every, **force_kw)
        return o.coords.astype(np.float64).copy(), o.vel.astype(np.float64).copy()
    return step


def constrained_step(o, cons, dt, remove_cm_every, general=False):
    from tests import constraints_ref as CR

    def step(x, v, first):
        return CR.vv_run(o, cons, x, v, 1, dt, remove_cm_every=remove_cm_every, first_step=first, general=general)
    return step


def sites_step(force_fn, cons, sites, m, box, dt, remove_cm_every):
    from tests import virtual_sites_ref as V

    def step(x, v, first):
        return V.vv_run(force_fn, cons, sites, x, v, m, box, 1, dt, remove_cm_every=remove_cm_every, first_step=first)
    return step
