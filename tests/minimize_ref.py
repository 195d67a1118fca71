"""simulate!(sys, ::SteepestDescentMinimizer) restated in numpy (simulators.jl:225-265), the checker of mhip_minimize: the loop over a force, an energy and
a placement function, and the twin of a constrained case that carries the constraints as harmonic bonds (constraints_to_bonds, constraints.jl:619-636)."""
import copy
import math

import numpy as np


def wrap(x, box):
    return x - box * np.floor(x / box)


def loop(x0, force_fn, energy_fn, step_size, max_steps, tol, dtype=np.float64, box=None, place_fn=None, wrap_fn=None):
    """x += (hn·F)/max‖F‖ in `dtype`, accepted when the energy falls (hn·6/5), taken back otherwise (hn/5), until max‖F‖ < tol.
    force_fn(x) → (n, 3) total forces with the sites' rows distributed; energy_fn(x) → float; place_fn(x) → x with the sites placed.
    One deviation from the reference, as the engine's: max‖F‖ == 0 moves nothing and stops.
    → dict(coords, accepted=[bool…], hn, E0, E, E_trial=[…], max_force=[…], hn_used=[…])"""
    T = np.dtype(dtype).type
    wrap_fn = wrap_fn or ((lambda x: wrap(x, np.asarray(box, dtype=dtype))) if box is not None else (lambda x: x))
    place_fn = place_fn or (lambda x: x)
    x = place_fn(wrap_fn(np.asarray(x0, dtype=dtype).copy()))
    E = E0 = float(energy_fn(x))
    hn = T(step_size)
    out = dict(accepted=[], E_trial=[], max_force=[], hn_used=[])
    for _ in range(max_steps):
        F = np.asarray(force_fn(x), dtype=dtype)
        max_force = np.sqrt((F * F).sum(axis=1, dtype=dtype)).max()
        keep = x.copy()
        if max_force != 0:
            x = place_fn(wrap_fn(x + (hn * F / max_force).astype(dtype)))
        E_trial = float(energy_fn(x))
        out["E_trial"].append(E_trial); out["max_force"].append(float(max_force)); out["hn_used"].append(float(hn))
        if E_trial < E:
            hn = T(6) * hn / T(5); E = E_trial; out["accepted"].append(True)
        else:
            x = keep; hn = hn / T(5); out["accepted"].append(False)
        if max_force < tol or max_force == 0:
            break
    out.update(coords=x, hn=float(hn), E0=E0, E=E)
    return out


def constrained_pairs(case):
    """(i, j, d) of every constrained pair: the distance constraints, and all three sides of an angle constraint (d_ik by the law of cosines, as AngleConstraint)"""
    c = case.constraints or {}
    i, j, d = [], [], []
    if c.get("dist") is not None:
        i += list(map(int, c["dist"]["i"])); j += list(map(int, c["dist"]["j"])); d += list(map(float, c["dist"]["d"]))
    a = c.get("angle")
    if a is not None:
        for ai, aj, ak, th, dij, djk in zip(a["i"], a["j"], a["k"], a["theta"], a["d_ij"], a["d_jk"]):
            dij, djk = float(dij), float(djk)
            dik = math.sqrt(dij ** 2 + djk ** 2 - 2 * dij * djk * math.cos(float(th)))
            i += [int(ai), int(aj), int(ai)]; j += [int(aj), int(ak), int(ak)]; d += [dij, djk, dik]
    return np.asarray(i, np.int32), np.asarray(j, np.int32), np.asarray(d, np.float64)


def twin_with_bonds(case, k):
    """the same case WITHOUT constraints and with one harmonic bond of constant k per constrained pair appended (k None: none appended); the same exclusions"""
    t = copy.copy(case)
    t.constraints = None
    if k is None:
        return t
    i, j, d = constrained_pairs(case)
    b = case.bonds
    t.bonds = dict(i=np.concatenate([np.asarray(b["i"], np.int32), i]) if b else i, j=np.concatenate([np.asarray(b["j"], np.int32), j]) if b else j,
                   k=np.concatenate([np.asarray(b["k"], np.float64), np.full(len(i), float(k))]) if b else np.full(len(i), float(k)),
                   r0=np.concatenate([np.asarray(b["r0"], np.float64), d]) if b else d)
    return t


def pair_deviation(case, coords):
    """largest | r − d | over the constrained pairs at `coords` (nearest image in the cubic box)"""
    i, j, d = constrained_pairs(case)
    dx = coords[j] - coords[i]
    dx -= case.box * np.round(dx / case.box)
    return float(np.abs(np.linalg.norm(dx, axis=1) - d).max())
