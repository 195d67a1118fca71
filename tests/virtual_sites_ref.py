"""Virtual sites restated in fp64 numpy (the checker of the engine's site kernels and of the step loops that host sites): placement and
force distribution (virtual.jl:187-294), velocity Verlet and Langevin with sites in the reference's order (simulators.jl:547-629,
1099-1220: place behind SHAKE and the wrap, distribute behind every force evaluation, no acceleration, noise or centre-of-mass
subtraction for a site), and the four-site water box the GPU tests run.  Constraints come from constraints_ref."""
import json
import os

import numpy as np

from tests import constraints_ref as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# a site: (type, atom_ind, atom_1, atom_2, atom_3, weight_1, weight_2, weight_3, weight_12, weight_13, weight_cross), 0-based, −1 unused
def site_arrays(sites):
    """→ (type, site, a1, a2, a3 int32 arrays, w6 flat float64) as mhip_set_virtual_sites takes them"""
    s = [tuple(v) for v in sites]
    cols = [np.ascontiguousarray([v[k] for v in s], dtype=np.int32) for k in range(5)]
    return (*cols, np.ascontiguousarray([v[5:11] for v in s], dtype=np.float64).reshape(-1))


def flags(n, sites):
    f = np.zeros(n, bool)
    f[[v[1] for v in sites]] = True
    return f


def _wrap(x, box):
    return x - box * np.floor(x / box)


def place(x, box, sites):
    """place_virtual_sites!: only r1 is absolute, the other parents enter as nearest-image vectors from it; the site is wrapped"""
    x = np.array(x, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    for t, s, a1, a2, a3, w1, w2, w3, w12, w13, wc in sites:
        r = x[a1].copy()
        if t >= 2:
            r12 = CR.min_image(x[a2] - x[a1], box)
        if t >= 3:
            r13 = CR.min_image(x[a3] - x[a1], box)
        if t == 2:
            r += w2 * r12
        elif t == 3:
            r += w2 * r12 + w3 * r13
        elif t == 4:
            r += w12 * r12 + w13 * r13 + wc * np.cross(r12, r13)
        x[s] = _wrap(r, box)
    return x


def distribute(f, x, box, sites):
    """distribute_forces!: each site's force onto its parents by the transposed Jacobian of place(); the site's row is zeroed"""
    f = np.array(f, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    for t, s, a1, a2, a3, w1, w2, w3, w12, w13, wc in sites:
        fs = f[s].copy()
        if t == 1:
            f[a1] += fs
        elif t == 2:
            f[a1] += w1 * fs; f[a2] += w2 * fs
        elif t == 3:
            f[a1] += w1 * fs; f[a2] += w2 * fs; f[a3] += w3 * fs
        else:
            r12 = CR.min_image(x[a2] - x[a1], box); r13 = CR.min_image(x[a3] - x[a1], box)
            f2 = w12 * fs + wc * np.cross(r13, fs)
            f3 = w13 * fs + wc * np.cross(fs, r12)
            f[a1] += fs - f2 - f3; f[a2] += f2; f[a3] += f3
        f[s] = 0.0
    return f


def lj_all_pairs(x, box, sigma, eps, excluded=()):
    """(forces, potential energy) of LennardJones without cutoff over every pair but the excluded ones (nearest image)"""
    n = len(x)
    box = np.asarray(box, dtype=np.float64)
    i, j = np.triu_indices(n, 1)
    keep = np.ones(len(i), bool)
    ex = {(min(a, b), max(a, b)) for a, b in excluded}
    for k, (a, b) in enumerate(zip(i.tolist(), j.tolist())):
        if (a, b) in ex:
            keep[k] = False
    i, j = i[keep], j[keep]
    dr = CR.min_image(x[j] - x[i], box)
    r2 = (dr * dr).sum(1)
    s2 = sigma * sigma / r2
    six = s2 * s2 * s2                                            # (products, not `**`: numpy's vectorised pow differs between CPUs by more than the bars here)
    fmag = 24.0 * eps / r2 * (2.0 * six * six - six)              # F/r
    f = np.zeros((n, 3))
    np.add.at(f, j, fmag[:, None] * dr)
    np.add.at(f, i, -fmag[:, None] * dr)
    return f, float((4.0 * eps * (six * six - six)).sum())


def oracle_forces(o, general=False):
    return lambda x: CR._forces(o, x, general)


class _NoConstraints:
    def rattle(self, x, v):
        pass

    def shake(self, x0, x):
        return 0


def _remove_cm(v, m, vsf):
    vcm = (m[:, None] * v).sum(0) / m.sum()
    v[~vsf] -= vcm


def vv_run(force_fn, cons, sites, x, v, m, box, n_steps, dt, remove_cm_every=1, first_step=0):
    """simulate!(sys, VelocityVerlet) with virtual sites (and constraints, or None); force_fn(x) → raw per-atom forces"""
    cons = cons or _NoConstraints()
    box = np.asarray(box, dtype=np.float64); m = np.asarray(m, dtype=np.float64)
    vsf = flags(len(m), sites)
    im = np.where(m > 0, 1.0 / np.where(m > 0, m, 1.0), 0.0)[:, None]
    x = place(_wrap(np.array(x, dtype=np.float64), box), box, sites); v = np.array(v, dtype=np.float64)
    if first_step == 0 and remove_cm_every:
        _remove_cm(v, m, vsf)
    a = distribute(force_fn(x), x, box, sites) * im
    for step in range(first_step + 1, first_step + n_steps + 1):
        v += a * (dt / 2)
        cons.rattle(x, v)
        x0 = x.copy()
        x += v * dt * (~vsf)[:, None]
        xu = x.copy()
        cons.shake(x0, x)
        v += (x - xu) / dt
        x = place(_wrap(x, box), box, sites)
        a = distribute(force_fn(x), x, box, sites) * im
        v += a * (dt / 2)
        cons.rattle(x, v)
        if remove_cm_every and step % remove_cm_every == 0:
            _remove_cm(v, m, vsf)
    return x, v


def langevin_run(force_fn, cons, sites, x, v, m, box, n_steps, dt, kT, friction, key, ctr1, randn3, remove_cm_every=1, first_step=0):
    """simulate!(sys, Langevin) with virtual sites; randn3(i, key, ctr1) → the three normals of atom i (OracleSystem.randn3)"""
    cons = cons or _NoConstraints()
    box = np.asarray(box, dtype=np.float64); m = np.asarray(m, dtype=np.float64)
    vsf = flags(len(m), sites)
    im = np.where(m > 0, 1.0 / np.where(m > 0, m, 1.0), 0.0)[:, None]
    x = place(_wrap(np.array(x, dtype=np.float64), box), box, sites); v = np.array(v, dtype=np.float64)
    vs = np.exp(-dt * friction); pref = np.sqrt(1.0 - vs * vs) * np.sqrt(kT)
    ns = np.where((m > 0) & ~vsf, pref * np.sqrt(1.0 / np.where(m > 0, m, 1.0)), 0.0)
    move = (~vsf)[:, None]
    if first_step == 0 and remove_cm_every:
        _remove_cm(v, m, vsf)
    for step in range(first_step + 1, first_step + n_steps + 1):
        a = distribute(force_fn(x), x, box, sites) * im
        v += a * dt
        cons.rattle(x, v)
        x0 = x.copy()
        x += v * (dt / 2) * move
        z = np.array([randn3(i, key, ctr1) for i in range(len(m))])
        ctr1 += 1
        v = np.where(move, vs * v + z * ns[:, None], v)
        x += v * (dt / 2) * move
        xu = x.copy()
        cons.shake(x0, x)
        v += (x - xu) / dt
        x = place(_wrap(x, box), box, sites)
        if remove_cm_every and step % remove_cm_every == 0:
            _remove_cm(v, m, vsf)
    return x, v


# ---- the reference's 13-atom toy (tests/golden/virtual_sites_basic.json) ---------------------------------------------------------------
def toy():
    g = json.load(open(os.path.join(GOLDEN, "virtual_sites_basic.json")))
    g["sites"] = [(s["type"], s["atom_ind"], s["atom_1"], s["atom_2"], s["atom_3"], *s["weights"]) for s in g["virtual_sites"]]
    for k in ("coords", "coords_true", "fs_true"):
        g[k] = np.asarray(g[k], dtype=np.float64)
    g["flags"] = np.asarray(g["virtual_site_flags"], bool)
    g["mass"] = np.where(g["flags"], g["mass_site"], g["mass_atom"]).astype(np.float64)
    return g


def toy_case(g=None, r_list=float("inf")):
    from molly_jl_amd.workloads import Case
    g = g or toy()
    n = len(g["coords"])
    return Case(g["coords_true"], g["box"], lj=dict(cutoff=("none",)), r_list=r_list, velocities=np.zeros((n, 3)), charge=np.zeros(n),
                sigma=np.full(n, g["sigma"]), eps=np.full(n, g["eps"]), mass=g["mass"], excluded=np.asarray(g["excluded"], dtype=np.int32),
                name="virtual_site_toy", virtual_sites=g["sites"])


# ---- four-site water -------------------------------------------------------------------------------------------------------------------
def tip4p_fb():
    return json.load(open(os.path.join(GOLDEN, "tip4p_fb.json")))


def _rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def tip4p_box(n_side, rigid=True, coulomb="rf", seed=11, three_site=False, temperature=300.0):
    """n_side³ TIP4P-FB waters (O, H1, H2, M) on a 0.31 nm lattice: one common orientation, each water turned by a random rotation of at
    most 20° and shifted by ±0.01 nm; exclusions for every intramolecular pair.  rigid: an angle constraint per water (the three
    distances), else harmonic bonds and angle.  coulomb: "rf" (reaction field, 0.9 nm) or "pme".  three_site: the same box without M,
    its charge on O (constraints only)."""
    from molly_jl_amd.workloads import Case
    w = tip4p_fb()
    rng = np.random.default_rng(seed)
    spacing = 0.31
    b, th = w["bond_length"], w["angle"]
    body = np.array([[0.0, 0.0, 0.0], [b * np.sin(th / 2), 0.0, b * np.cos(th / 2)], [-b * np.sin(th / 2), 0.0, b * np.cos(th / 2)]])
    base = _rotation(np.array([1.0, 2.0, 0.5]), 0.7)
    per = 3 if three_site else 4
    n_w = n_side ** 3
    x = np.zeros((n_w * per, 3))
    sites = []
    ws = w["site"]
    for c, cell in enumerate(np.ndindex(n_side, n_side, n_side)):
        R = _rotation(rng.normal(size=3), rng.uniform(0.0, np.deg2rad(20.0))) @ base
        o = (np.asarray(cell) + 0.5) * spacing + rng.uniform(-0.01, 0.01, 3)
        k = per * c
        x[k:k + 3] = o + body @ R.T
        if not three_site:
            sites.append((3, k + 3, k, k + 1, k + 2, ws["weight_1"], ws["weight_2"], ws["weight_3"], 0.0, 0.0, 0.0))
    names = ["O", "H", "H"] + ([] if three_site else ["M"])
    col = lambda key: np.tile(np.array([w[key][a] for a in names], dtype=np.float64), n_w)
    q, sig, eps, m = col("charge"), col("sigma"), col("eps"), col("mass")
    if three_site:
        q[0::3] = w["charge"]["M"]
    box = np.full(3, n_side * spacing)
    x = place(_wrap(x, box), box, sites)
    v = rng.normal(size=(len(x), 3)) * np.where(m > 0, np.sqrt(8.314462618e-3 * temperature / np.where(m > 0, m, 1.0)), 0.0)[:, None]
    first = per * np.arange(n_w)
    excl = np.array([(f + a, f + c) for f in first.tolist() for a in range(per) for c in range(a + 1, per)], dtype=np.int32)
    d_hh = float(np.sqrt(2 * b * b - 2 * b * b * np.cos(th)))
    kw = {}
    if rigid:
        kw["constraints"] = dict(angle=dict(i=(first + 1).astype(np.int32), j=first.astype(np.int32), k=(first + 2).astype(np.int32),
                                            theta=np.full(n_w, th), d_ij=np.full(n_w, b), d_jk=np.full(n_w, b)))
    else:
        kw["bonds"] = dict(i=np.concatenate([first, first]).astype(np.int32), j=np.concatenate([first + 1, first + 2]).astype(np.int32),
                           k=np.full(2 * n_w, w["bond_k"]), r0=np.full(2 * n_w, b))
        kw["angles"] = dict(i=(first + 1).astype(np.int32), j=first.astype(np.int32), k=(first + 2).astype(np.int32), kth=np.full(n_w, w["angle_k"]), th0=np.full(n_w, th))
    rc = min(0.9, 0.35 * float(box[0]))
    if coulomb == "pme":
        coul = dict(kind="ewald", rc=rc); kw["pme"] = dict(order=5); kw["ewald_excl"] = excl
    else:
        coul = dict(kind="rf", rc=rc, eps_rf=78.3)
    case = Case(x, box, lj=dict(cutoff=("distance", rc)), coul=coul, r_list=rc + 0.2, rebuild_every=10, velocities=v, charge=q, sigma=sig, eps=eps, mass=m,
                excluded=excl, name=f"tip4p_{n_side}" + ("_3site" if three_site else ""), **(dict(virtual_sites=sites) if sites else {}), **kw)
    case.d_hh = d_hh
    return case


def min_intermolecular_distance(case, per=4):
    """smallest atom–atom distance between different waters of a tip4p_box start (nearest image)"""
    x, box = case.coords, case.box
    mol = np.arange(case.n) // per
    best = np.inf
    for a in range(0, case.n, 512):
        d = CR.min_image(x[a:a + 512, None, :] - x[None, :, :], box)
        r = np.sqrt((d * d).sum(-1))
        r[mol[a:a + 512, None] == mol[None, :]] = np.inf
        best = min(best, float(r.min()))
    return best
