"""One nonbonded pair, restated in numpy: force factor, energy and virial of LennardJones, Coulomb, CoulombReactionField and CoulombEwald under
the six cutoff strategies, evaluated entirely in a chosen dtype (np.float32, np.float64, np.longdouble).  Independent of oracle/: tests/test_pair_host.py
pins this file to the oracle and to the reference's known answers before tests/test_gpu_pair_physics.py lets it judge a kernel.

Behavioural spec (Molly.jl v0.23.3), the same lines as the header of csrc/physics.h:
    lennard_jones.jl:79-140    F = (24ϵ/r)(2 s6² − s6), V = 4ϵ(s6² − s6), s6 = (σ²/r²)³; × weight_special for a special pair
    coulomb.jl:71-120          F = ke qi qj / r², V = ke qi qj / r
    coulomb.jl:748-814         reaction field: F/r = kqq (1/r − 2 krf r²)/r², V = kqq (1/r + krf r² − crf); krf = crf = 0 for a special pair
    coulomb.jl:1384-1441       Ewald direct space: F/r = kqq/r³ · (erfc(αr) + 2αr·exp(−α²r²)/√π), V = kqq/r · erfc(αr); a special pair: plain Coulomb × weight
    cutoffs.jl:15-253          None, Distance, ShiftedPotential, ShiftedForce, CubicSpline, Polynomial; `r <= rc` and `r <= ra` are inclusive
    mixing.jl:3-34             σ = (σi + σj)/2, ϵ = √(ϵi ϵj); LJZeroShortcut: σ = 0 or ϵ = 0 of either atom gives 0
    spatial.jl:491-551         the displacement from atom i to atom j (cubic compare/select form; triclinic: the nearest of the 27 images)
The force on atom j is fr·dr and −fr·dr on atom i (force.jl:873-874); a pair adds dr ⊗ (fr·dr) to the virial (force.jl:848-852).

Inputs (coordinates, per-atom parameters, radii, weights, α) are numbers of the precision the system under test runs in (`param_dtype`); the arithmetic on
them runs in `dtype`.  The exact erfc is math.erfc — double precision at every dtype, so the longdouble reference of an exact-erfc case is a double in that one factor."""
import math

import numpy as np

from tests import systems as S

KE = 138.93545764          # coulomb.jl:16
CUTOFFS = ("none", "distance", "shifted_potential", "shifted_force", "cubic_spline", "polynomial")


def _erfc_exact(x, T):
    return np.array([math.erfc(float(v)) for v in np.ravel(x)], dtype=T).reshape(np.shape(x))


# ---- bare potentials: (F(r), V(r)) ------------------------------------------------------------------------
def lj_bare(r, s2, e):
    six = (s2 / (r * r)) ** 3
    return (24 * e / r) * (2 * six * six - six), 4 * e * (six * six - six)


def coul_bare(r, kqq):
    return kqq / (r * r), kqq * (1 / r)


# ---- cutoffs.jl on a bare potential `bare(r) -> (F, V)` ---------------------------------------------------
def apply_cutoff(kind, rc, ra, bare, r):
    """(F_c(r), V_c(r)) of one of the six strategies; rc, ra are scalars of r's dtype"""
    T = r.dtype.type
    f, v = bare(r)
    if kind == "none":
        return f, v
    zero = np.zeros_like(r)
    inside = r <= rc
    if kind == "distance":
        return np.where(inside, f, zero), np.where(inside, v, zero)
    one = np.ones_like(r)
    if kind == "shifted_potential":
        _, vc = bare(rc * one)
        return np.where(inside, f, zero), np.where(inside, v - vc, zero)
    if kind == "shifted_force":
        fc, vc = bare(rc * one)
        return np.where(inside, f - fc, zero), np.where(inside, v + (r - rc) * fc - vc, zero)
    fa, va = bare(ra * one)
    w = rc - ra
    t = (r - ra) / w
    if kind == "cubic_spline":
        dva = -fa
        fs = -(6 * t ** 2 - 6 * t) * va / w - (3 * t ** 2 - 4 * t + 1) * dva
        vs = (2 * t ** 3 - 3 * t ** 2 + 1) * va + (t ** 3 - 2 * t ** 2 + t) * w * dva
    elif kind == "polynomial":
        sw = 1 - 6 * t ** 5 + 15 * t ** 4 - 10 * t ** 3
        dsw = (-30 * t ** 4 + 60 * t ** 3 - 30 * t ** 2) / w
        fs = sw * f - dsw * v
        vs = sw * v
    else:
        raise ValueError(kind)
    active = r <= ra
    return np.where(active, f, np.where(inside, fs, zero)).astype(T), np.where(active, v, np.where(inside, vs, zero)).astype(T)


def _cut(c, P, T):
    """('kind', rc[, ra]) with the radii as numbers of the parameter precision P, held in T"""
    kind = c[0]
    rc = T(P(c[1])) if len(c) > 1 else T(0)
    ra = T(P(c[2])) if len(c) > 2 else T(0)
    return kind, rc, ra


def ewald_alpha(rc, tol, P):
    """α = √(−log(2 tol))/rc in the parameter precision (coulomb.jl:1332), as workloads.Case.inter_dict and api.CoulombEwald derive it"""
    return float((P(1) / P(rc)) * np.sqrt(-np.log(P(2) * P(tol))))


def erfc_as(ar, ex, T):
    """calc_erfc with approximate_erfc (coulomb.jl:1384-1393): Abramowitz & Stegun 7.1.26"""
    t = 1 / (1 + T(0.3275911) * ar)
    return (T(0.254829592) + (T(-0.284496736) + (T(1.421413741) + (T(-1.453152027) + T(1.061405429) * t) * t) * t) * t) * t * ex


def pair(lj, coul, dr, qi, qj, si, sj, ei, ej, special, dtype, param_dtype=None, dr_is_exact=False):
    """Force factor, energy and magnitude scales of pairs i→j, every operation in `dtype`.
    lj, coul: the interaction dicts of workloads.Case; dr (n, 3); per-atom parameters (n,); special (n,) bool.
    → dict(fr, pe, S, E): the force on j is fr·dr; S = 24ϵ(2s¹² + s⁶)/r + |kqq|/r² and E = 4ϵ(s¹² + s⁶) + |kqq|/r are the bare magnitudes of the active
    interactions (no cutoff, no weight): the scales an error is measured against, since LJ crosses zero at 2^(1/6)σ and at σ."""
    T = np.dtype(dtype).type
    P = np.dtype(param_dtype or (np.float64 if T is np.longdouble else dtype)).type
    inp = lambda a: np.asarray(a, dtype=np.float64).astype(P).astype(T)      # an input: a number of the parameter precision
    dr = (np.asarray(dr, dtype=T) if dr_is_exact else inp(dr)).reshape(-1, 3)      # (dr_is_exact: already a displacement of this dtype, not an input to round)
    qi, qj, si, sj, ei, ej = (inp(a) for a in (qi, qj, si, sj, ei, ej))
    special = np.asarray(special, dtype=bool)
    r2 = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]
    r = np.sqrt(r2)
    fr, pe, Sc, Ec = (np.zeros_like(r) for _ in range(4))
    if lj is not None:
        kind, rc, ra = _cut(lj.get("cutoff", ("none",)), P, T)
        w = np.where(special, T(P(lj.get("weight_special", 1.0))), T(1))
        live = (si != 0) & (sj != 0) & (ei != 0) & (ej != 0)                   # LJZeroShortcut
        s = (si + sj) / 2
        e = np.sqrt(ei * ej)
        s = np.where(live, s, T(1)); e = np.where(live, e, T(0))
        f, v = apply_cutoff(kind, rc, ra, lambda x: lj_bare(x, s * s, e), r)
        fr = fr + np.where(live, (f / r) * w, T(0))
        pe = pe + np.where(live, v * w, T(0))
        s6 = np.where(live, (s * s / r2) ** 3, T(0))
        Sc = Sc + 24 * e * (2 * s6 * s6 + s6) / r
        Ec = Ec + 4 * e * (s6 * s6 + s6)
    if coul is not None:
        ke = T(P(KE))
        kqq = ke * qi * qj
        w = np.where(special, T(P(coul.get("weight_special", 1.0))), T(1))
        k = coul["kind"]
        if k == "plain":
            kind, rc, ra = _cut(coul.get("cutoff", ("none",)), P, T)
            f, v = apply_cutoff(kind, rc, ra, lambda x: coul_bare(x, kqq), r)
            fr = fr + (f / r) * w
            pe = pe + v * w
        elif k == "rf":
            rc, eps = T(P(coul["rc"])), coul.get("eps_rf", 78.3)
            if math.isinf(eps):
                krf, crf = 1 / (2 * rc ** 3), 3 * (1 / (2 * rc))
            else:
                eps = T(P(eps))
                krf, crf = (1 / rc ** 3) * (eps - 1) / (2 * eps + 1), (1 / rc) * (3 * eps) / (2 * eps + 1)
            krf = np.where(special, T(0), T(krf)); crf = np.where(special, T(0), T(crf))
            inside = r <= rc
            f = kqq * (1 / r - 2 * krf * r2) * (1 / r2)
            fr = fr + np.where(inside, f * w, T(0))
            pe = pe + np.where(inside, kqq * (1 / r + krf * r2 - crf) * w, T(0))
        elif k == "ewald":
            rc = T(P(coul["rc"]))
            alpha = T(ewald_alpha(coul["rc"], coul.get("tol", 5e-4), P))
            inv_r = 1 / r
            ar = alpha * r
            ex = np.exp(-ar ** 2)
            ec = erfc_as(ar, ex, T) if coul.get("approx", True) else _erfc_exact(ar, T)
            pi = T(np.pi) if T is not np.longdouble else 4 * np.arctan(np.longdouble(1))
            inside = r <= rc
            f = kqq * inv_r ** 3
            g = ec + 2 * ar * ex / np.sqrt(pi)
            fr = fr + np.where(inside, np.where(special, f * w, f * g), T(0))
            pe = pe + np.where(inside, kqq * inv_r * np.where(special, w, ec), T(0))
        else:
            raise ValueError(k)
        Sc = Sc + np.abs(kqq) / r2
        Ec = Ec + np.abs(kqq) / r
    return dict(fr=fr.astype(T), pe=pe.astype(T), S=Sc.astype(T), E=Ec.astype(T), r=r, dr=dr)


# ---- displacement i → j with the boundary's arithmetic (spatial.jl:491-551) -------------------------------
def displacement(ci, cj, box, dtype, param_dtype, basis=None):
    T = np.dtype(dtype).type
    P = np.dtype(param_dtype).type
    inp = lambda a: np.asarray(a, dtype=np.float64).astype(P).astype(T)
    ci, cj = inp(ci).reshape(-1, 3), inp(cj).reshape(-1, 3)
    if basis is None:
        L = inp(box).reshape(1, 3)
        v = cj - ci
        vp, vm = v + L, v - L
        return np.where(v > 0, np.where(v < -vm, v, vm), np.where(-v < vp, v, vp))
    bv = inp(basis).reshape(3, 3)
    best = np.full(len(ci), np.inf, dtype=T)
    out = np.zeros_like(ci)
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                d = (cj + T(ox) * bv[0] + T(oy) * bv[1] + T(oz) * bv[2]) - ci
                sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                take = sq < best
                best = np.where(take, sq, best)
                out = np.where(take[:, None], d, out)
    return out


# ---- probe systems: isolated dimers ------------------------------------------------------------------------
# species: distinct σ, ϵ, q; three of them switch one interaction off each
SPECIES = {"A": (0.30, 0.80, 0.60), "B": (0.24, 0.40, -0.50), "eps0": (0.28, 0.0, 0.30), "sig0": (0.0, 0.50, -0.40), "q0": (0.26, 0.60, 0.0)}
SPECIES_PAIRS = (("A", "A"), ("A", "B"), ("B", "B"), ("A", "eps0"), ("B", "sig0"), ("A", "q0"), ("q0", "q0"), ("eps0", "q0"), ("sig0", "q0"))
FLAGS = ("plain", "special", "excluded")
R_LIST, RA_NOMINAL = 1.2, 0.8
DELTA = {np.dtype(np.float32): 2.0 ** -16, np.dtype(np.float64): 2.0 ** -40}
BAND = {np.dtype(np.float32): 4e-6, np.dtype(np.float64): 1e-13}
TRI_BASIS = np.array([[20.8, 0.0, 0.0], [2.6, 20.8, 0.0], [-1.3, 2.6, 20.8]])


def edges_of(lj, coul):
    """the radii at which some active interaction changes branch: {name: radius}"""
    e = {}
    for tag, c in (("lj", lj.get("cutoff") if lj else None), ("c", coul.get("cutoff") if coul and coul["kind"] == "plain" else None)):
        if c is not None and len(c) > 1:
            e.setdefault(float(c[1]), "rc")
            if len(c) > 2:
                e.setdefault(float(c[2]), "ra")
    if coul and coul["kind"] in ("rf", "ewald"):
        e.setdefault(float(coul["rc"]), "rc")
    if not e:
        e[1.0] = "rc"                                                  # nothing cuts: nominal radii keep the classes the same
    if not any(v == "ra" for v in e.values()):
        e.setdefault(RA_NOMINAL, "ra")
    return dict(sorted(e.items()))


def distance_classes(lj, coul):
    """[(name, kind, lo, hi or None)]: kind 'range' draws uniformly, 'edge-' / 'edge+' sit at radius·(1 ∓ δ)"""
    ed = edges_of(lj, coul)
    radii = list(ed)
    rc_max, ra_min = max(radii), min(radii)
    cls = [("core", "sigma", 0.85, 1.0), ("well", "sigma", 1.0, 2.0), ("mid", "mid", 2.0, ra_min)]
    for x in radii:
        cls += [(f"{ed[x]}{x:g}-", "edge-", x, None), (f"{ed[x]}{x:g}+", "edge+", x, None)]
    for lo, hi in zip(radii[:-1], radii[1:]):
        cls.append((f"switch{lo:g}_{hi:g}", "range", lo * 1.01, hi * 0.99))
    cls += [("gap", "range", rc_max * 1.01, R_LIST * 0.99), ("beyond", "range", R_LIST * 1.02, 1.35)]
    return cls


class Probe:
    """a probe system: the Case plus what each dimer was drawn as"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def probe_system(dtype, lj=None, coul=None, n_side=8, spacing=2.6, seed=1, only=None, uniform=False, flags=FLAGS, triclinic=None, species_pairs=SPECIES_PAIRS, cells=None):
    """Isolated dimers on a coarse lattice (n_side³ nodes `spacing` apart, box n_side·spacing, r_list 1.2): no atom of one dimer lies within r_list of another
    dimer's atom (asserted by brute force over the periodic images), so every atom has exactly one partner and an error belongs to one pair.  Lattice nodes sit
    ON the box faces, so the dimers of the first layers straddle them.  Each dimer draws a distance class (distance_classes), a species pair and a flag; the
    three are crossed (every (class, flag) cell holds at least 4 dimers when n_side = 8).  `only`: every dimer is of that one class (the energy / virial
    systems).  `uniform`: one atom type, no charges.  `cells`: the (class, flag) cells to deal the dimers to, for a system too small for the full crossing.  triclinic: None | dict(approx_images=…) — the lattice in the skewed basis TRI_BASIS·(n_side/8).
    Coordinates and parameters are rounded to `dtype`.  Asserts that every edge probe's distance, as rounded, is outside the band |r/radius − 1| < BAND[dtype]."""
    dt = np.dtype(dtype)
    T = dt.type
    rng = np.random.default_rng(seed)
    n_d = n_side ** 3
    classes = distance_classes(lj, coul)
    if only is not None:
        classes = [c for c in classes if c[0] == only]
        assert classes, only
    by_name = {c[0]: c for c in classes}
    cells = [(c, f) for c in classes for f in flags] if cells is None or only is not None else [(by_name[c], f) for c, f in cells]
    k = np.arange(n_d)
    cell_of = k % len(cells)
    sp_of = [("A", "A")] * n_d if uniform else [species_pairs[(i + i // len(cells)) % len(species_pairs)] for i in k]
    node = rng.permutation(n_d)
    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)[node]
    box_len = n_side * spacing
    basis = None
    if triclinic is not None:
        basis = TRI_BASIS * (n_side / 8.0)
        basis = basis.astype(T).astype(np.float64)
        centre = (g / n_side) @ basis
        box = np.diag(basis).copy()
    else:
        centre = g * spacing
        box = np.full(3, float(T(box_len)))
    u = rng.normal(size=(n_d, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    par = np.array([[SPECIES[a], SPECIES[b]] for a, b in sp_of])                     # (n_d, 2, 3): σ, ϵ, q
    if uniform:
        par[:, :, 2] = 0.0
    par = par.astype(T).astype(np.float64)
    lj_live = np.all(par[:, :, :2] != 0, axis=(1, 2)) & (lj is not None)
    smix = np.where(lj_live, 0.5 * (par[:, 0, 0] + par[:, 1, 0]), 0.3)              # the σ a class is measured in: the mixed σ, or a typical one where LJ is off
    delta = DELTA[dt]
    r = np.zeros(n_d)
    for i in k:
        (name, kind, lo, hi), _ = cells[cell_of[i]]
        if kind == "sigma":
            r[i] = rng.uniform(lo, hi) * smix[i]
        elif kind == "mid":
            r[i] = rng.uniform(lo * smix[i] * 1.001, hi * 0.99)
        elif kind == "range":
            r[i] = rng.uniform(lo, hi)
        else:
            r[i] = lo * (1 - delta if kind == "edge-" else 1 + delta)
    x = np.stack([centre - 0.5 * r[:, None] * u, centre + 0.5 * r[:, None] * u], 1).reshape(-1, 3)
    if basis is None:
        x = x - np.floor(x / box) * box
        x = x.astype(T).astype(np.float64)
        x = np.where(x >= box, 0.0, x)
    else:
        fr_ = np.linalg.solve(basis.T, x.T).T
        x = (fr_ - np.floor(fr_)) @ basis
        x = x.astype(T).astype(np.float64)
    n = 2 * n_d
    ia, ib = 2 * k, 2 * k + 1
    flag_of = np.array([cells[c][1] for c in cell_of])
    cls_of = np.array([cells[c][0][0] for c in cell_of])
    kind_of = np.array([cells[c][0][1] for c in cell_of])
    edge_of = np.array([cells[c][0][2] if cells[c][0][1].startswith("edge") else np.nan for c in cell_of])
    pairs = np.stack([ia, ib], 1)
    case = S.Case(x, box, lj=lj, coul=None if uniform else coul, r_list=R_LIST, rebuild_every=10, velocities=np.zeros((n, 3)),
                  charge=None if uniform else par[:, :, 2].reshape(-1), sigma=par[:, :, 0].reshape(-1), eps=par[:, :, 1].reshape(-1), mass=np.full(n, 12.0),
                  excluded=pairs[flag_of == "excluded"] if (flag_of == "excluded").any() else None,
                  special=pairs[flag_of == "special"] if (flag_of == "special").any() else None,
                  triclinic=None if triclinic is None else dict(basis=basis, approx_images=triclinic.get("approx_images", True)),
                  name=f"probe{n}")
    p = Probe(case=case, dtype=dt, ia=ia, ib=ib, flag=flag_of, cls=cls_of, kind=kind_of, edge=edge_of, species=sp_of, basis=basis, classes=[c[0] for c in classes],
              lj=lj, coul=None if uniform else coul)
    check_isolated(p)
    check_band(p)
    return p


GRID = 2.0 ** -10


def grid_probe_system(dtype, lj=None, coul=None, n_side=8, seed=3, uniform=False, flags=("plain", "special")):
    """Dimers at EXACTLY a cutoff radius.  Every coordinate, the lattice spacing (2664·2⁻¹⁰ = 2.6015625 nm) and the box (n_side spacings) are multiples of 2⁻¹⁰ nm, the dimers lie
    along ±x, ±y, ±z, and the radii of the cases that use this builder are binary fractions (1.0, 0.875): coordinate differences, block centres, block-local
    coordinates, periodic shifts and r² = (k·2⁻¹⁰)² are all exact in fp32 and fp64, so a dimer at r = rc has r² == rc² in the kernel as in the reference, and
    `r <= rc` INCLUDES it (cutoffs.jl:20, coulomb.jl:779, 1411) — which no probe a relative δ away from the radius can tell from `<`.  Classes per radius:
    'rc<x>=' at the radius, 'rc<x>=-' and 'rc<x>=+' one grid step inside / outside.  Nodes of the first layers put dimers across the box faces."""
    dt = np.dtype(dtype)
    T = dt.type
    rng = np.random.default_rng(seed)
    radii = [x for x, kind in edges_of(lj, None if uniform else coul).items() if kind == "rc"]
    assert all(float(x / GRID).is_integer() for x in radii), radii
    classes = [(f"rc{x:g}{tag}", x + off) for x in radii for tag, off in (("=", 0.0), ("=-", -GRID), ("=+", GRID))]
    cells = [(c, f) for c in classes for f in flags]
    n_d = n_side ** 3
    k = np.arange(n_d)
    cell_of = k % len(cells)
    sp_of = [("A", "A")] * n_d if uniform else [SPECIES_PAIRS[(i + i // len(cells)) % len(SPECIES_PAIRS)] for i in k]
    node = rng.permutation(n_d)
    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)[node]
    spacing = 2664 * GRID
    box = np.full(3, n_side * spacing)
    axis = rng.integers(0, 3, n_d); sign = rng.choice([-1.0, 1.0], n_d)
    r = np.array([cells[c][0][1] for c in cell_of])
    a = g * spacing + 0.25      # (a quarter nanometre off the faces: the dimers along an axis of the first layer still cross them, and no 64-atom block of the sorted atoms spans the box)
    a[k, axis] -= sign * 0.5
    b = a.copy()
    b[k, axis] += sign * r
    x = np.stack([a, b], 1).reshape(-1, 3)
    x = x - np.floor(x / box) * box
    assert np.all(x / GRID == np.round(x / GRID)) and np.array_equal(x, x.astype(T).astype(np.float64)) and x.min() >= 0 and x.max() < box[0]
    par = np.array([[SPECIES[p_], SPECIES[q_]] for p_, q_ in sp_of])
    if uniform:
        par[:, :, 2] = 0.0
    par = par.astype(T).astype(np.float64)
    n = 2 * n_d
    ia, ib = 2 * k, 2 * k + 1
    flag_of = np.array([cells[c][1] for c in cell_of])
    pairs = np.stack([ia, ib], 1)
    case = S.Case(x, box, lj=lj, coul=None if uniform else coul, r_list=R_LIST, rebuild_every=10, velocities=np.zeros((n, 3)),
                  charge=None if uniform else par[:, :, 2].reshape(-1), sigma=par[:, :, 0].reshape(-1), eps=par[:, :, 1].reshape(-1), mass=np.full(n, 12.0),
                  special=pairs[flag_of == "special"] if (flag_of == "special").any() else None, name=f"grid{n}")
    p = Probe(case=case, dtype=dt, ia=ia, ib=ib, flag=flag_of, cls=np.array([cells[c][0][0] for c in cell_of]), kind=np.array(["exact"] * n_d),
              edge=np.full(n_d, np.nan), species=sp_of, basis=None, classes=[c[0] for c in classes], lj=lj, coul=None if uniform else coul, radius=r)
    check_isolated(p)
    assert np.array_equal(p.r64, r)                                                   # the distances ARE the radii, to the last bit
    return p


def _all_image_dist2(x, box, basis):
    """(n, n) squared distance to the nearest image, in fp64: the orthorhombic minimum image, or the nearest of the 27 images of a skewed cell"""
    d = x[None, :, :] - x[:, None, :]
    if basis is None:
        d -= np.round(d / box) * box
        return np.einsum("ijk,ijk->ij", d, d)
    best = np.full((len(x), len(x)), np.inf)
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                e = d + (ox * basis[0] + oy * basis[1] + oz * basis[2])
                np.minimum(best, np.einsum("ijk,ijk->ij", e, e), out=best)
    return best


def check_isolated(p):
    """no atom of one dimer within r_list of another dimer's atom, over every periodic image — and no image of its own partner closer than the partner"""
    x = p.case.coords
    d2 = _all_image_dist2(x, p.case.box, p.basis)
    own = (np.arange(len(x))[:, None] // 2) == (np.arange(len(x))[None, :] // 2)
    other = np.where(own, np.inf, d2)
    assert other.min() > (R_LIST + 0.03) ** 2, f"dimers not isolated: nearest foreign atom at {math.sqrt(other.min()):.4f} nm"
    p.r64 = np.sqrt(d2[p.ia, p.ib])
    return p.r64


def check_band(p):
    """every edge probe, as rounded to the dtype, is clearly on its side of the radius: the kernel's own rounding of r² cannot flip it"""
    m = ~np.isnan(p.edge)
    if m.any():
        rel = p.r64[m] / p.edge[m] - 1.0
        assert np.all(np.abs(rel) >= BAND[p.dtype]), f"edge probe inside the band: min |r/rc − 1| = {np.abs(rel).min():.3e}"
        want = np.where(p.kind[m] == "edge-", -1.0, 1.0)
        assert np.all(np.sign(rel) == want)
    return True


def dimer_reference(p, dtype, stretch=0.0, exact_dr=False):
    """the probe system's dimers through displacement() and pair() at `dtype`: dict(fr, pe, S, E, dr, r, f (force on atom j = ib, (n_d, 3)), vir (n_d, 3, 3),
    listed) — an excluded dimer and one beyond r_list contribute nothing.  stretch: every displacement lengthened by that many nm along itself (the
    sensitivity probes of reference_errors).  exact_dr: the displacement is taken at longdouble and rounded once to `dtype` — the pair formula's own arithmetic alone."""
    c = p.case
    dr = displacement(c.coords[p.ia], c.coords[p.ib], c.box, np.longdouble if (exact_dr or stretch) else dtype, p.dtype, p.basis)
    if stretch:
        dr = dr * (1 + np.longdouble(stretch) / np.sqrt((dr * dr).sum(axis=1)))[:, None]
    q = c.charge if c.charge is not None else np.zeros(c.n)
    special = p.flag == "special"
    T = np.dtype(dtype).type
    out = pair(p.lj, p.coul, dr.astype(T), q[p.ia], q[p.ib], c.sigma[p.ia], c.sigma[p.ib], c.eps[p.ia], c.eps[p.ib], special, dtype, p.dtype, dr_is_exact=True)
    listed = (p.r64 <= R_LIST) & (p.flag != "excluded")
    out["listed"] = listed
    for key in ("fr", "pe"):
        out[key] = np.where(listed, out[key], T(0))
    out["f"] = out["fr"][:, None] * out["dr"]
    out["vir"] = out["fr"][:, None, None] * out["dr"][:, :, None] * out["dr"][:, None, :]
    return out


def reference_errors(p, dtype):
    """The error budget of a probe system's dimers at `dtype`, from the reference's own arithmetic: dict(ref, S, E, W, bar_f, bar_e, bar_w, …), the bars per
    unit of the path's factor k (tests/test_gpu_pair_physics.py): a dimer's force bar is  min(k·Ef·S, k·Ea·S + Df)  (energy: Ee, Eae, De; virial: Ew, Eaw, Dw).
      Ef  the worst |pair_ref(dtype) − pair_ref(longdouble)|/S over the system's listed dimers, displacement arithmetic included — the bar's definition.
          Its largest term is no pair formula: c2 − c1 across the box is rounded at the size of the BOX (half an ulp of 20.8 nm: 1e-6 nm in fp32), and a core
          dimer feels δr as 13·δr/r of its force.  Only dimers across a face meet it in the reference; in a kernel that shifts each atom into a block-local
          frame any dimer may.  So the budget is split, and is never wider than k·Ef:
      Ea  the same worst error with the displacement given (taken at longdouble, rounded once): the pair formula's arithmetic alone, over every listed dimer;
      Df  per dimer, how far its force moves when the displacement is off by u = √3·½ulp(L) along itself (the steepest direction), at longdouble: ONE rounding
          at the size of the box, as the reference's own displacement has (measured on the MI355X: with two allowed the bars had more than 3× slack)."""
    lo, hi, ar = dimer_reference(p, dtype), dimer_reference(p, np.longdouble), dimer_reference(p, dtype, exact_dr=True)
    c = p.case
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    S_, E_, r_ = f64(hi["S"]), f64(hi["E"]), f64(hi["r"])
    raw = c.coords[p.ib] - c.coords[p.ia]
    p.straddles = np.abs(raw - f64(hi["dr"])).max(axis=1) > 1e-3
    u = math.sqrt(3.0) * 0.5 * float(np.spacing(p.dtype.type(np.max(c.box if p.basis is None else np.abs(p.basis).sum(axis=0)))))
    m = hi["listed"] & (S_ > 0)
    dist = lambda a, b, key, red: red(np.abs(f64(a[key].astype(np.longdouble) - b[key])))
    vec = lambda x: np.linalg.norm(x.reshape(len(x), -1), axis=1) if x.ndim == 2 else (x.reshape(len(x), -1).max(axis=1) if x.ndim == 3 else x)
    out = dict(ref=hi, S=S_, E=E_, W=S_ * r_, u=u)
    scale = {"f": S_, "pe": E_, "vir": S_ * r_}
    for key, tag in (("f", "f"), ("pe", "e"), ("vir", "w")):
        worst = lambda a: float((dist(a, hi, key, vec)[m] / scale[key][m]).max()) if m.any() else 0.0
        full, arith = worst(lo), worst(ar)
        D = np.maximum(*(dist(dimer_reference(p, np.longdouble, stretch=sg * u), hi, key, vec) for sg in (1.0, -1.0)))
        if getattr(p, "arith_from", None) is not None:      # (grid probes, see grid_probe: no cap by their own all-but-exact arithmetic)
            arith = reference_errors(p.arith_from, dtype)["Ea" + tag]; full = np.inf; D = np.zeros_like(D)      # … and no rounding of a displacement: on the grid it is exact
        out["E" + tag], out["Ea" + tag], out["D" + tag] = full, arith, D
        out["bar_" + tag] = lambda k, full=full, arith=arith, D=D, sc=scale[key]: np.minimum(k * full * sc, k * arith * sc + D) if np.isfinite(full) else k * arith * sc + D
    return out


def sum_allowance(terms):
    """what adding up n numbers one after the other in double precision may cost, worst case: n·2⁻⁵³·Σ|term| (the engine sums every atom's share — each pair
    from both ends — in double, the oracle the pairs; neither is part of a pair's own error budget)"""
    t = np.abs(np.asarray(terms, dtype=np.float64))
    return 2 * t.shape[0] * 2.0 ** -53 * float(t.sum(axis=0).max())


def structural_zero(p):
    """the dimers whose force must be exactly zero, from how they were drawn — not from evaluating anything: excluded, beyond the list, or every active
    interaction either switched off by the species (σ = 0 / ϵ = 0 / q = 0) or past the radius at which its strategy cuts"""
    c = p.case
    r = p.r64
    off = np.ones(len(r), bool)
    if p.lj is not None:
        live = (c.sigma[p.ia] != 0) & (c.sigma[p.ib] != 0) & (c.eps[p.ia] != 0) & (c.eps[p.ib] != 0)
        cut = p.lj.get("cutoff", ("none",))
        off &= ~live | ((r > cut[1]) if cut[0] != "none" else False)
    if p.coul is not None:
        live = (c.charge[p.ia] != 0) & (c.charge[p.ib] != 0)
        if p.coul["kind"] == "plain":
            cut = p.coul.get("cutoff", ("none",))
            off &= ~live | ((r > cut[1]) if cut[0] != "none" else False)
        else:
            off &= ~live | (r > p.coul["rc"])
    return off | (p.flag == "excluded") | (r > R_LIST)


def jump_probes(p):
    """The dimers just inside a radius where the FORCE has a finite jump, and whose species make that jump the bulk of the pair's force: a wrong inclusion
    there loses a force far above any bar.  LennardJones under Distance / ShiftedPotential: the pairs without charge (next to a Coulomb force of 50 kJ/mol/nm the
    LJ jump of 0.01 is within fp32 round-off); Coulomb under the same two strategies, the reaction field with a finite dielectric, Ewald direct space: the
    charged pairs.  (ShiftedForce, CubicSpline, Polynomial and the conducting reaction field, 1 − 2 krf rc³ = 0, are continuous in the force; NoCutoff does not cut.)"""
    c = p.case
    m = np.zeros(len(p.r64), bool)
    q = c.charge if c.charge is not None else np.zeros(c.n)
    charged = (q[p.ia] != 0) & (q[p.ib] != 0) & (p.coul is not None)
    exact_r = getattr(p, "radius", np.full(len(p.r64), np.inf))
    at = lambda x: ((p.kind == "edge-") & (p.edge == x)) | ((p.kind == "exact") & (exact_r <= x) & (exact_r >= x - GRID))     # (grid probes: AT the radius and one step inside)
    if p.lj is not None and p.lj.get("cutoff", ("none",))[0] in ("distance", "shifted_potential"):
        live = (c.sigma[p.ia] != 0) & (c.sigma[p.ib] != 0) & (c.eps[p.ia] != 0) & (c.eps[p.ib] != 0)
        m |= live & ~charged & at(p.lj["cutoff"][1])
    if p.coul is not None:
        if p.coul["kind"] == "plain":
            cut = p.coul.get("cutoff", ("none",))
            if cut[0] in ("distance", "shifted_potential"):
                m |= charged & at(cut[1])
        elif p.coul["kind"] == "ewald" or not math.isinf(p.coul.get("eps_rf", 78.3)):
            m |= charged & at(p.coul["rc"])
    return m & (p.flag != "excluded")


# ---- the cases of tests/test_pair_host.py and tests/test_gpu_pair_physics.py --------------------------------------------------------------------
def _cut_of(kind, rc=1.0, ra=0.8):
    return (kind,) if kind == "none" else ((kind, rc, ra) if kind in ("cubic_spline", "polynomial") else (kind, rc))


W14 = 0.8333333333333334
LJ_DIST = dict(cutoff=("distance", 1.0), weight_special=0.5)
COUL = {"rf": dict(kind="rf", rc=1.0, eps_rf=78.3, weight_special=W14), "rf_inf": dict(kind="rf", rc=1.0, eps_rf=math.inf, weight_special=W14),
        "ewald": dict(kind="ewald", rc=1.0, approx=True, weight_special=W14), "ewald_exact": dict(kind="ewald", rc=1.0, approx=False, weight_special=W14)}
SMALL_CELLS = (("core", "plain"), ("well", "special"), ("mid", "plain"), ("switch0.8_1", "plain"), ("rc1-", "plain"), ("rc1-", "special"), ("rc1+", "plain"), ("gap", "excluded"))
CASES = {}
for _k in CUTOFFS:
    CASES[f"lj_{_k}"] = dict(lj=dict(cutoff=_cut_of(_k), weight_special=0.5), coul=None)
    CASES[f"coul_{_k}"] = dict(lj=LJ_DIST, coul=dict(kind="plain", cutoff=_cut_of(_k), weight_special=W14))
for _k in ("lj_none", "coul_none"):      # NoCutoff over a list keeps the single list with its finer cell grid; on 1 024 atoms in a 20.8 nm box a 64-atom block's
    CASES[_k]["n_side"] = 5              # neighbourhood then spans more cells than the search kernel's table holds (MHIP_ERR_CAPACITY).  125 dimers in 13 nm: ≥ 4 per cell still.
CASES["lj_uniform"] = dict(lj=LJ_DIST, coul=None, uniform=True, flags=("plain", "excluded"))
CASES["lj_uniform_special"] = dict(lj=LJ_DIST, coul=None, uniform=True)
for _k, _c in COUL.items():
    CASES[_k] = dict(lj=LJ_DIST, coul=_c)
for _k in ("rf", "ewald"):
    CASES[f"mismatch_{_k}"] = dict(lj=dict(cutoff=("distance", 0.9), weight_special=0.5), coul=COUL[_k])
    CASES[f"small_{_k}"] = dict(lj=LJ_DIST, coul=COUL[_k], n_side=2, cells=SMALL_CELLS)
    for _a in (True, False):
        CASES[f"tri_{_k}_{'approx' if _a else 'images'}"] = dict(lj=LJ_DIST, coul=COUL[_k], triclinic=dict(approx_images=_a))
BOTH = [n for n in CASES if not n.startswith(("mismatch", "tri"))]
FP32_ONLY = [n for n in CASES if n.startswith(("mismatch", "tri"))]
GPU_CASES = [(n, np.float32) for n in CASES] + [(n, np.float64) for n in BOTH]      # every (case, precision) the GPU tests run

# dimers at exactly the cutoff: the cases whose force jumps at a binary-fraction radius (the two-cutoff launch with lj_rc = 0.875 for 0.9)
GRID_CASES = {n: CASES[n] for n in ("lj_distance", "lj_shifted_potential", "coul_distance", "coul_shifted_potential", "lj_uniform_special", "rf", "ewald", "ewald_exact")}
GRID_CASES["lj_uniform"] = dict(CASES["lj_uniform"], flags=("plain",))
for _k in ("rf", "ewald"):
    GRID_CASES[f"mismatch_{_k}"] = dict(lj=dict(cutoff=("distance", 0.875), weight_special=0.5), coul=COUL[_k])
    GRID_CASES[f"small_{_k}"] = dict(lj=LJ_DIST, coul=COUL[_k], n_side=2)
GRID_GPU_CASES = [(n, d) for d in (np.float32, np.float64) for n in GRID_CASES]

_probes = {}


def grid_probe(name, dtype):
    key = ("grid", name, np.dtype(dtype))
    if key not in _probes:
        _probes[key] = grid_probe_system(dtype, **GRID_CASES[name])
        # At r² = 1 exactly most of the reference's own operations are exact, so its error THERE says nothing about a kernel that hoists σ² and 24ϵ or asks the
        # 1-ulp units: the formula's arithmetic error is taken from the case's random-orientation system (mismatch: the 0.9 / 1.0 one), and that is the whole bar.
        _probes[key].arith_from = probe(name if name in CASES else name.replace("small_", ""), dtype)
    return _probes[key]



def probe(name, dtype, only=None):
    """the probe system of a named case (built once): the full crossed system, or — `only` — the small one whose dimers are all of one distance class"""
    key = (name, np.dtype(dtype), only)
    if key not in _probes:
        kw = dict(CASES[name])
        if only is not None:
            kw["n_side"] = min(kw.get("n_side", 8), 4)
        _probes[key] = probe_system(dtype, only=only, **kw)
    return _probes[key]
