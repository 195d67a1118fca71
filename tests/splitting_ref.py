"""numpy restatement of simulate!(sys, ::LangevinSplitting) (simulators.jl:1255-1398) and simulate!(sys, ::OverdampedLangevin) (:1426-1489), the checker of
mhip_splitting_run and mhip_overdamped_run.  It drives an oracle instance (oracle/pyoracle.py) for everything that is not the integrator — o.forces, o.neighbors,
o.wrap, o.remove_cm, o.randn3 — and works in place on o.coords / o.vel, in the precision of the instance it is given: every product and sum below is one numpy
operation on arrays of that dtype, so each is rounded once, as the reference's broadcasts are.  The O sub-step's scales are evaluated in double from the atom's mass
and rounded once (the convention of the engine's thermal_scale); its multiply-add is fused, as langevin_o_step_kernel! writes it (kernels.jl:739)."""
import re

import numpy as np


def plan(splitting, dt):
    """→ dict(dts, force, forces_known_at_start, segments): simulators.jl:1305-1324 by the reference's regex and loop; segments = [begin, end) runs that end in
    front of a force-computing B or at the end of the step"""
    if not splitting or any(c not in "ABO" for c in splitting):
        raise ValueError("splitting must contain only A, B, and O steps")              # :1276-1278
    dts = [dt / splitting.count(c) for c in splitting]                                  # :1305
    known = re.search(r"^.*B[^B]*A[^B]*$", splitting) is None                           # :1308
    at_start, force = known, []
    for c in splitting:                                                                 # :1310-1324
        if c == "O":
            force.append(False)
        elif c == "A":
            known = False; force.append(False)
        elif known:
            force.append(False)
        else:
            known = True; force.append(True)
    cuts = [0] + [j for j in range(1, len(splitting)) if force[j]] + [len(splitting)]
    return dict(dts=dts, force=force, forces_known_at_start=at_start, segments=list(zip(cuts[:-1], cuts[1:])))


def _fma(a, b, c):
    """a·b + c rounded once (fp32: exactly, through double; fp64: two roundings — an ulp, far inside every bar here)"""
    if c.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def _normals(o, key, ctr1, rows):
    z = np.zeros((o.n, 3), o.dtype)
    for i in rows:
        z[i] = o.randn3(int(i), key, ctr1 % 2 ** 64)                                    # (0-based index: the generator's ctr0 is i + 1)
    return z


def _lists(o, nthreads):
    return o.neighbors("cell", nthreads=nthreads) if np.isfinite(o.r_list) and o.r_list > 0 else None


def splitting_run(o, n_steps, dt, kT, friction, splitting, key=0, ctr1=0, first_step=0, remove_cm_every=1, nthreads=1, **force_kw):
    """friction: mass per time.  Returns the number of force evaluations inside the loop."""
    T = o.dtype.type
    P = plan(splitting, dt)
    m64 = o.mass.astype(np.float64)
    massive = m64 != 0
    rows = np.nonzero(massive)[0]
    inv_m = np.zeros(o.n, o.dtype); inv_m[massive] = T(1) / o.mass[massive]             # M_inv, 0 for a virtual site (:1272-1275)
    n_o = splitting.count("O")
    vel_scale = np.ones(o.n, o.dtype); noise_scale = np.zeros(o.n, o.dtype)
    if n_o:
        a = (friction * dt / n_o) / m64[massive]                                        # :1282
        vel_scale[massive] = np.exp(-a).astype(o.dtype)
        noise_scale[massive] = np.sqrt(kT / m64[massive] * (1.0 - np.exp(-2.0 * a))).astype(o.dtype)   # :1286-1289
    every = o.rebuild_every if o.rebuild_every > 0 else 10
    o.wrap()                                                                            # :1294
    if first_step == 0 and remove_cm_every != 0:
        o.remove_cm()                                                                   # :1296
    nl = _lists(o, nthreads)                                                            # :1297
    f = o.forces(nl, nthreads=nthreads, **force_kw) if P["forces_known_at_start"] and "B" in splitting else None      # :1302 (used by a B only)
    n_force = 0
    for step in range(first_step + 1, first_step + n_steps + 1):
        for j, op in enumerate(splitting):
            h = T(P["dts"][j])
            if op == "A":                                                               # A_step!, :1383-1388
                o.coords += o.vel * h
                o.wrap()
            elif op == "B":                                                             # B_step!, :1390-1398
                if P["force"][j]:
                    f = o.forces(nl, nthreads=nthreads, **force_kw); n_force += 1
                o.vel += h * (f * inv_m[:, None])
            else:                                                                       # langevin_o_step!, kernels.jl:726-741
                z = _normals(o, key, ctr1, rows)
                ctr1 += 1                                                               # :1355
                new = _fma(np.broadcast_to(vel_scale[:, None], o.vel.shape), o.vel, noise_scale[:, None] * z)
                o.vel[massive] = new[massive]
        if remove_cm_every != 0 and step % remove_cm_every == 0:
            o.remove_cm()                                                               # :1365-1367
        if nl is not None and step % every == 0:
            nl = _lists(o, nthreads)                                                    # :1369
    return n_force


def overdamped_run(o, n_steps, dt, kT, gamma, key=0, ctr1=0, first_step=0, remove_cm_every=1, nthreads=1, **force_kw):
    """gamma: inverse time.  One key and a counter that advances by one per step (the engine's convention; the reference draws a fresh pair per step).
    remove_CM_motion! once, when the call starts at step 0 or holds a due step: the velocities never change."""
    T = o.dtype.type
    m64 = o.mass.astype(np.float64)
    massive = m64 != 0
    rows = np.nonzero(massive)[0]
    inv_m = np.zeros(o.n, o.dtype); inv_m[massive] = T(1) / o.mass[massive]
    scale = np.zeros(o.n, o.dtype); scale[massive] = (np.sqrt(kT) * np.sqrt(1.0 / m64[massive])).astype(o.dtype)      # random_velocities!: sqrt(kT/m)·ξ
    prefac = T(np.sqrt((2.0 / gamma) * dt))                                             # :1454
    every = o.rebuild_every if o.rebuild_every > 0 else 10
    last = first_step + n_steps
    o.wrap()                                                                            # :1444
    if remove_cm_every != 0 and (first_step == 0 or last // remove_cm_every > first_step // remove_cm_every):
        o.remove_cm()                                                                   # :1446, :1471-1473
    nl = _lists(o, nthreads)                                                            # :1447
    for step in range(first_step + 1, last + 1):
        f = o.forces(nl, nthreads=nthreads, **force_kw)                                 # :1461
        noise = _normals(o, key, ctr1 + (step - first_step - 1), rows) * scale[:, None]  # :1464
        move = ((f * inv_m[:, None]) / T(gamma)) * T(dt) + prefac * noise               # :1465
        o.coords[massive] += move[massive]
        o.wrap()                                                                        # :1466
        if nl is not None and step % every == 0:
            nl = _lists(o, nthreads)                                                    # :1475
