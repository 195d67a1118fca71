"""A second opinion on the specific interactions (HarmonicBond, HarmonicAngle, PeriodicTorsion, EwaldExclusion) — plain numpy, TEST INFRASTRUCTURE ONLY.

The device kernels (csrc/bonded.h) and the oracle (oracle/oracle.cpp) both carry the reference's closed-form force expressions; an error the two share would
pass every parity test.  This module holds the four ENERGIES only, written from their definitions, and derives everything else from them numerically:

  bond       k/2 (r − r0)²                        angle      k/2 (θ − θ0)²,   θ the angle between r_i − r_j and r_k − r_j
  torsion    k + k cos(nφ − phase)                exclusion  −ke·qi·qj·erf(αr)/r  (→ −2α·ke·qi·qj/√π as r → 0)

forces()  = −∂E/∂x by central differences, virial() = −∂E/∂ε under a symmetric strain of box and coordinates together, per_atom_scale() = Σ over the terms of an
atom of the norm of that term's force on it.  No force formula appears here.  Works in float64 or np.longdouble (x87 extended: 64-bit mantissa).

Also the synthetic systems of tests/test_bonded_host.py and tests/test_gpu_bonded.py (chains(), hub(), …), so that the CPU-side checks of the reference and
the device tests see the same inputs."""
import math

import numpy as np

from tests import systems as S

KE = 138.93545764          # coulomb.jl:16
ROLES = {"bonds": ("i", "j"), "angles": ("i", "j", "k"), "torsions": ("i", "j", "k", "l"), "excl": ("i", "j")}
TYPES = ("bonds", "angles", "torsions", "excl")
H_FD = 1e-5                # nm / strain: step of the 4th-order central difference (see fd())
H_NEAR = 1e-7              # … for the angles 1e-3 and 1e-5 rad off collinear, whose energy bends on the scale of the off-axis offset (1e-4 … 1e-6 nm)


def _pi(T):
    return T(4) * np.arctan(T(1))


def _inv3(b):
    """inverse of a 3×3 matrix by cofactors, in the matrix' own precision (np.linalg has no longdouble)"""
    c = np.empty_like(b)
    for i in range(3):
        for j in range(3):
            m = [[b[(i + 1 + p) % 3, (j + 1 + q) % 3] for q in range(2)] for p in range(2)]
            c[j, i] = m[0][0] * m[1][1] - m[0][1] * m[1][0]
    return c / (b[0, 0] * c[0, 0] + b[0, 1] * c[1, 0] + b[0, 2] * c[2, 0])


def _erf_over_x(x, T):
    """erf(x)/x = 2/√π · e^{−x²} · Σ_n 2ⁿ x^{2n} / (2n+1)!!  — positive terms only, exact at x = 0, converged to longdouble for x < 4"""
    x2 = x * x
    term = np.ones_like(x2); s = np.ones_like(x2)
    for n in range(1, 160):
        term = term * (T(2) * x2) / T(2 * n + 1)
        s = s + term
    return T(2) / np.sqrt(_pi(T)) * np.exp(-x2) * s


class Ref:
    """the specific interactions of a Case as term tables; every method takes the coordinates and the cell (rows = basis vectors) as arguments"""

    def __init__(self, case, dtype=np.float64):
        T = self.T = np.dtype(dtype).type
        self.n = case.n
        self.x = np.asarray(case.coords, dtype=T)
        basis = np.diag(case.box) if case.triclinic is None else np.asarray(case.triclinic["basis"], dtype=np.float64).reshape(3, 3)
        self.basis = np.asarray(basis, dtype=T)
        f = lambda a: np.asarray(a, dtype=np.float64).astype(T)
        self.idx, self.par = {}, {}
        if case.bonds is not None and len(case.bonds["i"]):
            self.idx["bonds"] = np.stack([case.bonds["i"], case.bonds["j"]], 1).astype(np.int64); self.par["bonds"] = (f(case.bonds["k"]), f(case.bonds["r0"]))
        if case.angles is not None and len(case.angles["i"]):
            a = case.angles
            self.idx["angles"] = np.stack([a["i"], a["j"], a["k"]], 1).astype(np.int64); self.par["angles"] = (f(a["kth"]), f(a["th0"]))
        if case.torsions is not None and len(case.torsions["i"]):
            t = case.torsions
            self.idx["torsions"] = np.stack([t["i"], t["j"], t["k"], t["l"]], 1).astype(np.int64); self.par["torsions"] = (f(t["periodicity"]), f(t["phase"]), f(t["k0"]))
        if case.ewald_excl is not None and len(case.ewald_excl):
            e = np.asarray(case.ewald_excl, dtype=np.int64).reshape(-1, 2)
            q = f(case.charge)
            self.idx["excl"] = e; self.par["excl"] = (q[e[:, 0]] * q[e[:, 1]],)
            self.alpha = T(case.inter_dict(np.float64)["ewald_alpha"])

    # -- geometry ------------------------------------------------------------------------------------------
    def image(self, d, basis):
        """the shortest lattice image of the displacements d (m, 3): wrap the fractional coordinates, then try the 27 cells around"""
        s = d @ _inv3(basis)
        d = (s - np.round(s)) @ basis
        best, best2 = d, (d * d).sum(axis=1)
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                for c in (-1, 0, 1):
                    if a == b == c == 0:
                        continue
                    e = d + (self.T(a) * basis[0] + self.T(b) * basis[1] + self.T(c) * basis[2])
                    e2 = (e * e).sum(axis=1)
                    m = e2 < best2
                    best = np.where(m[:, None], e, best); best2 = np.where(m, e2, best2)
        return best

    def term_energies(self, ty, p, basis):
        """energies of the terms of one type; p (m, roles, 3) = the terms' own atom coordinates"""
        T = self.T
        nrm = lambda v: np.sqrt((v * v).sum(axis=1))
        if ty == "bonds":
            k, r0 = self.par[ty]
            r = nrm(self.image(p[:, 1] - p[:, 0], basis))
            return k / T(2) * (r - r0) ** 2
        if ty == "angles":
            k, th0 = self.par[ty]
            u, w = self.image(p[:, 0] - p[:, 1], basis), self.image(p[:, 2] - p[:, 1], basis)
            th = np.arctan2(nrm(np.cross(u, w)), (u * w).sum(axis=1))      # the angle between u and w, well conditioned at 0 and π
            return k / T(2) * (th - th0) ** 2
        if ty == "torsions":
            per, phase, k = self.par[ty]
            ab, bc, cd = (self.image(p[:, q + 1] - p[:, q], basis) for q in range(3))
            n1, n2 = np.cross(ab, bc), np.cross(bc, cd)
            phi = np.arctan2((np.cross(n1, n2) * bc).sum(axis=1) / nrm(bc), (n1 * n2).sum(axis=1))
            return k + k * np.cos(per * phi - phase)
        (qq,) = self.par[ty]
        r = nrm(self.image(p[:, 1] - p[:, 0], basis))
        return -T(KE) * qq * self.alpha * _erf_over_x(self.alpha * r, T)

    def _xb(self, x, basis):
        return (self.x if x is None else np.asarray(x, dtype=self.T)), (self.basis if basis is None else np.asarray(basis, dtype=self.T))

    def energy(self, x=None, basis=None):
        x, basis = self._xb(x, basis)
        return sum((self.term_energies(ty, x[self.idx[ty]], basis).sum() for ty in self.idx), self.T(0))

    # -- derivatives ---------------------------------------------------------------------------------------
    def fd(self, fun, h=H_FD):
        """4th-order central difference of fun at 0: (8 (f(h) − f(−h)) − (f(2h) − f(−2h))) / 12h.  In longdouble with h = 1e-5 nm the truncation term h⁴ E⁽⁵⁾/30
        is below 1e-12 of the derivative for every term here (the stiffest, a bond or an exclusion at 1/64 nm, has E⁽⁵⁾/E' ≈ 24/r⁴ ≈ 4e8 nm⁻⁴) and the
        rounding term ε·E/h about 1e-14·E/nm; in float64 rounding dominates (1e-11·E/nm), which is what the float64 mode is for: showing that."""
        h = self.T(h)
        return (self.T(8) * (fun(h) - fun(-h)) - (fun(h + h) - fun(-h - h))) / (self.T(12) * h)

    def term_forces(self, x=None, basis=None, h=H_FD):
        """{type: (m, roles, 3)}: −∂(term energy)/∂(coordinate of the term's atom in that role)"""
        x, basis = self._xb(x, basis)
        out = {}
        for ty, idx in self.idx.items():
            p = x[idx]
            f = np.zeros_like(p)
            for r in range(idx.shape[1]):
                for d in range(3):
                    def e(s):
                        q = p.copy(); q[:, r, d] += s
                        return self.term_energies(ty, q, basis)
                    f[:, r, d] = -self.fd(e, h)
            out[ty] = f
        return out

    def forces(self, x=None, basis=None, h=H_FD):
        """−∂E/∂x per coordinate by central differences.  E is a sum of terms and the difference quotient is linear, so the quotient of E for a coordinate is the
        sum of the quotients of the terms that hold the atom: taken per term (three coordinates of every term at once), then added per atom."""
        f = np.zeros((self.n, 3), self.T)
        for ty, tf in self.term_forces(x, basis, h).items():
            for r in range(tf.shape[1]):
                np.add.at(f, self.idx[ty][:, r], tf[:, r])
        return f

    def per_atom_scale(self, x=None, basis=None, h=H_FD):
        """S_i = Σ over the terms atom i takes part in of ‖that term's force on i‖: the size of what is summed into f_i, the yardstick of every per-atom bar"""
        s = np.zeros(self.n, self.T)
        for ty, tf in self.term_forces(x, basis, h).items():
            for r in range(tf.shape[1]):
                np.add.at(s, self.idx[ty][:, r], np.sqrt((tf[:, r] ** 2).sum(axis=1)))
        return s

    def virial_scale(self, x=None, basis=None, h=H_FD):
        """Σ over the terms and their atoms of ‖r_atom − r_first‖·‖f_atom‖: the size of what a term's virial is made of, for geometry where the tensor itself
        all but vanishes (planar torsions)"""
        x, basis = self._xb(x, basis)
        tot = self.T(0)
        for ty, tf in self.term_forces(x, basis, h).items():
            p = x[self.idx[ty]]
            for r in range(1, tf.shape[1]):
                d = self.image(p[:, r] - p[:, 0], basis)
                tot += (np.sqrt((d * d).sum(axis=1)) * np.sqrt((tf[:, r] ** 2).sum(axis=1))).sum()
        return float(tot)

    def virial(self, x=None, basis=None, h=H_FD):
        """W_ab = −∂E/∂ε_ab for the symmetric strain ε = s (e_a e_bᵀ + e_b e_aᵀ)/2 applied as x → (1 + ε) x to coordinates and cell together (α fixed, as the
        Ewald splitting parameter is a constant of the interaction).  Equals the symmetric part of Σ r ⊗ f."""
        x, basis = self._xb(x, basis)
        w = np.zeros((3, 3), self.T)
        for a in range(3):
            for b in range(a, 3):
                def e(s):
                    F = np.eye(3, dtype=self.T)
                    F[a, b] += s / self.T(2); F[b, a] += s / self.T(2)
                    return self.energy(x @ F.T, basis @ F.T)
                w[a, b] = w[b, a] = -self.fd(e, h)
        return w


def of_case(case, dtype=np.longdouble):
    return Ref(case, dtype)


def energy(case, dtype=np.longdouble):
    return of_case(case, dtype).energy()


def forces(case, dtype=np.longdouble, h=H_FD):
    return of_case(case, dtype).forces(h=h)


def virial(case, dtype=np.longdouble, h=H_FD):
    return of_case(case, dtype).virial(h=h)


def per_atom_scale(case, dtype=np.longdouble, h=H_FD):
    return np.asarray(of_case(case, dtype).per_atom_scale(h=h), dtype=np.float64)


# ---- systems ---------------------------------------------------------------------------------------------------
TRI_BASIS = np.array([[4.0, 0.0, 0.0], [0.25, 4.0, 0.0], [0.5, 0.75, 4.0]])      # (exactly representable in fp32)


def _place(a, b, c, bond, theta, phi):
    """the next atom of a chain from its three predecessors: |cd| = bond, angle(b, c, d) = theta, dihedral(a, b, c, d) = phi"""
    bc = c - b; bc /= np.linalg.norm(bc)
    n = np.cross(b - a, bc); n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d2 = np.array([-bond * math.cos(theta), bond * math.sin(theta) * math.cos(phi), bond * math.sin(theta) * math.sin(phi)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * n


def _chain_coords(rng, m):
    """m atoms: bond lengths 0.1–0.2 nm, bond angles 1.2–2.6 rad, dihedrals anywhere — nothing degenerate, by construction and checked below"""
    x = [np.zeros(3), np.array([rng.uniform(0.1, 0.2), 0.0, 0.0])]
    th = rng.uniform(1.2, 2.6); b = rng.uniform(0.1, 0.2)
    x.append(x[1] + b * np.array([-math.cos(th), math.sin(th), 0.0]))
    for _ in range(3, m):
        x.append(_place(x[-3], x[-2], x[-1], rng.uniform(0.1, 0.2), rng.uniform(1.2, 2.6), rng.uniform(-math.pi, math.pi)))
    x = np.array(x[:m])
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))        # a random orientation
    return x @ q.T


def _regular(x, topo_chains, basis):
    """the drawing rule of the regular systems, measured on the coordinates the tests use (after rounding to fp32 and wrapping)"""
    inv = np.linalg.inv(basis)
    def mi(d):
        s = d @ inv; return (s - np.round(s)) @ basis
    for ch in topo_chains:
        p = x[ch]
        b = mi(p[1:] - p[:-1]); r = np.linalg.norm(b, axis=1)
        if r.min() < 0.0999 or r.max() > 0.2001:
            return False
        if len(ch) >= 3:
            cs = -(b[:-1] * b[1:]).sum(axis=1) / (r[:-1] * r[1:]); th = np.arccos(np.clip(cs, -1, 1))
            if th.min() < 1.199 or th.max() > 2.601 or np.abs(np.sin(th)).min() <= 0.3:
                return False
    return True


def chains(n_bonds=0, n_angles=0, n_torsions=0, n_excl=0, seed=0, box=8.0, triclinic=False, chain_len=6, n_free=None, lj=False, dtype=np.float32):
    """Independent chains of `chain_len` atoms spread over the whole cell (they cross its faces), carrying EXACTLY the asked number of terms of each type — each
    chain gives what is still missing of every type it can hold (bonds i–i+1, angles, torsion entries, exclusions i–i+1 and i–i+2) — plus n_free atoms without any
    term (default: as many as make the atom count odd, so it is never a multiple of 32).  Every system has charges and an Ewald direct-space Coulomb (rc 1.0; the
    exclusion terms read its α), with lj=True also per-atom LJ parameters and a 1.0 nm cutoff.  Coordinates are rounded to `dtype` and wrapped into the cell."""
    rng = np.random.default_rng([seed, n_bonds, n_angles, n_torsions, n_excl])
    basis = TRI_BASIS if triclinic else np.diag(np.full(3, float(box)))
    want = dict(bonds=n_bonds, angles=n_angles, torsions=n_torsions, excl=n_excl)
    have = dict.fromkeys(want, 0)
    terms = {ty: [] for ty in want}
    xs, topo = [], []
    n = 0
    while any(have[ty] < want[ty] for ty in want):
        m = chain_len
        ids = np.arange(n, n + m)
        cand = dict(bonds=[(ids[q], ids[q + 1]) for q in range(m - 1)], angles=[(ids[q], ids[q + 1], ids[q + 2]) for q in range(m - 2)],
                    torsions=[(ids[q], ids[q + 1], ids[q + 2], ids[q + 3]) for q in range(m - 3)],
                    excl=[(ids[q], ids[q + 1]) for q in range(m - 1)] + [(ids[q], ids[q + 2]) for q in range(m - 2)])
        for ty in want:
            take = cand[ty][:want[ty] - have[ty]]
            terms[ty] += take; have[ty] += len(take)
        for _ in range(100):
            xc = _chain_coords(rng, m) + rng.uniform(0, 1, 3) @ basis
            xc = xc.astype(dtype).astype(np.float64)
            if _regular(xc, [np.arange(m)], basis):
                break
        else:
            raise RuntimeError("no regular chain drawn")
        xs.append(xc); topo.append(ids); n += m
    if n_free is None:
        n_free = 1 if n % 2 == 0 else 2
    x = np.concatenate(xs + [rng.uniform(0, 1, (n_free, 3)) @ basis])
    s = x @ np.linalg.inv(basis); x = ((s - np.floor(s)) @ basis).astype(dtype).astype(np.float64)
    n = len(x)
    assert n % 32 != 0 and _regular(x, topo, basis)
    kw = {}
    A = lambda ty: np.array(terms[ty], dtype=np.int64).reshape(len(terms[ty]), -1)
    r32 = lambda a: np.asarray(a).astype(dtype).astype(np.float64)      # parameters every precision can hold
    if n_bonds:
        t = A("bonds"); r = _dist(x, t[:, 0], t[:, 1], basis)
        kw["bonds"] = dict(i=t[:, 0], j=t[:, 1], k=r32(rng.uniform(1e5, 3e5, len(t))), r0=r32(r + rng.choice([-1, 1], len(t)) * rng.uniform(0.005, 0.02, len(t))))
    if n_angles:
        t = A("angles")
        kw["angles"] = dict(i=t[:, 0], j=t[:, 1], k=t[:, 2], kth=r32(rng.uniform(300, 600, len(t))), th0=r32(rng.uniform(1.6, 2.2, len(t))))
    if n_torsions:
        t = A("torsions")
        kw["torsions"] = dict(i=t[:, 0], j=t[:, 1], k=t[:, 2], l=t[:, 3], periodicity=rng.integers(1, 7, len(t)), phase=r32(rng.uniform(-math.pi, math.pi, len(t))),
                              k0=r32(rng.uniform(0.5, 5.0, len(t))))
    if n_excl:
        kw["ewald_excl"] = A("excl"); kw["excluded"] = A("excl")
    q = rng.normal(size=n) * 0.4
    rc = 1.0
    case = S.Case(x, np.diag(basis), coul=dict(kind="ewald", rc=rc), r_list=1.2, charge=r32(q), mass=np.full(n, 12.0), velocities=np.zeros((n, 3)),
                  lj=dict(cutoff=("distance", rc)) if lj else None, sigma=np.full(n, 0.2) if lj else None, eps=np.full(n, 0.5) if lj else None,
                  triclinic=dict(basis=basis) if triclinic else None, name=f"chains_b{n_bonds}_a{n_angles}_t{n_torsions}_x{n_excl}", **kw)
    case.topo_chains = topo
    return case


def _dist(x, i, j, basis):
    inv = np.linalg.inv(basis)
    s = (x[j] - x[i]) @ inv
    return np.linalg.norm((s - np.round(s)) @ basis, axis=1)


def only(case, *types):
    """a copy of a case that keeps the named term types only (the charges, the Coulomb interaction and the pair exclusions stay)"""
    import copy
    c = copy.copy(case)
    if "bonds" not in types: c.bonds = None
    if "angles" not in types: c.angles = None
    if "torsions" not in types: c.torsions = None
    if "excl" not in types: c.ewald_excl = None
    return c


def n_terms(case):
    return dict(bonds=0 if case.bonds is None else len(case.bonds["i"]), angles=0 if case.angles is None else len(case.angles["i"]),
                torsions=0 if case.torsions is None else len(case.torsions["i"]), excl=0 if case.ewald_excl is None else len(np.asarray(case.ewald_excl).reshape(-1, 2)))


def bead_chain():
    """the 60-bead chain of tests/test_gpu_parity.py::test_bonded_terms_match_oracle: bonds, angles, torsions (2 Fourier terms each) and Ewald exclusions"""
    rng = np.random.default_rng(6)
    n = 60
    x = np.cumsum(rng.normal(size=(n, 3)) * 0.09 + np.array([0.08, 0.02, 0.01]), axis=0) + 3.0
    idx = np.arange(n)
    bonds = dict(i=idx[:-1], j=idx[1:], k=np.full(n - 1, 250000.0), r0=np.full(n - 1, 0.15))
    angles = dict(i=idx[:-2], j=idx[1:-1], k=idx[2:], kth=np.full(n - 2, 400.0), th0=np.full(n - 2, 1.9))
    ti = np.repeat(idx[:-3], 2)
    tors = dict(i=ti, j=ti + 1, k=ti + 2, l=ti + 3, periodicity=np.tile([1, 3], n - 3), phase=np.tile([0.0, math.pi], n - 3), k0=np.tile([2.5, 0.7], n - 3))
    ewx = np.concatenate([np.stack([idx[:-1], idx[1:]], 1), np.stack([idx[:-2], idx[2:]], 1)])
    q = rng.normal(size=n) * 0.4
    return S.Case(x, 8.0, coul=dict(kind="ewald", rc=1.0), r_list=1.2, charge=q, excluded=ewx, bonds=bonds, angles=angles, torsions=tors, ewald_excl=ewx)


HUB_ROLES = (("bonds", 0), ("angles", 1), ("torsions", 2), ("excl", 1), ("torsions", 0), ("angles", 0), ("bonds", 1), ("torsions", 3), ("angles", 2), ("torsions", 1), ("excl", 0))


def hub(m, mixed, seed=0, lj=True, dtype=np.float32):
    """One hub atom (index 0) that takes part in exactly m term slots, and half as many atoms again as the terms use that take part in none (a third of the system),
    scattered within 0.9 nm of the hub so that they do have pair partners.  mixed=False: m bonds hub–satellite.  mixed=True: the hub takes the roles of HUB_ROLES in
    turn, a fresh short chain per term with the hub at that place of it — from m = 11 on it sits in every role of every type; below that in the first m of them (all
    four types from m = 4) — and bonds make up the rest of m.  Every chain is drawn by the rule of the regular systems.  The cluster straddles two faces of the box."""
    rng = np.random.default_rng([seed, m, int(mixed)])
    basis = np.diag(np.full(3, 8.0))
    c = np.array([0.02, 7.99, 4.0])
    plan = list(HUB_ROLES[:min(m, 11)]) + [("bonds", q % 2) for q in range(max(m - 11, 0))] if mixed else [("bonds", q % 2) for q in range(m)]
    xs, terms, topo = [c], {ty: [] for ty in TYPES}, []
    for ty, role in plan:
        k = len(ROLES[ty])
        while True:
            xc = _chain_coords(rng, k)
            xc = (xc - xc[role] + c).astype(dtype).astype(np.float64)
            if _regular(xc, [np.arange(k)], basis):
                break
        ids, nxt = [], sum(len(a) for a in xs[1:]) + 1
        for q in range(k):
            if q == role: ids.append(0)
            else: ids.append(nxt); nxt += 1
        xs.append(np.delete(xc, role, axis=0)); terms[ty].append(ids); topo.append(np.array(ids))
    x = np.concatenate([xs[0][None]] + xs[1:])
    n_with = len(x)
    n_free = n_with // 2
    while (n_with + n_free) % 32 == 0 or n_free * 3 < n_with + n_free - 2: n_free += 1
    u = rng.normal(size=(n_free, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    x = np.concatenate([x, c + u * rng.uniform(0.4, 0.9, (n_free, 1))])
    x = (x - np.floor(x / 8.0) * 8.0).astype(dtype).astype(np.float64)
    n = len(x)
    assert _regular(x, topo, basis)
    r32 = lambda a: np.asarray(a).astype(dtype).astype(np.float64)
    kw = {}
    if terms["bonds"]:
        t = np.array(terms["bonds"]); r = _dist(x, t[:, 0], t[:, 1], basis)
        kw["bonds"] = dict(i=t[:, 0], j=t[:, 1], k=r32(rng.uniform(1e5, 3e5, len(t))), r0=r32(r + rng.choice([-1, 1], len(t)) * rng.uniform(0.005, 0.02, len(t))))
    if terms["angles"]:
        t = np.array(terms["angles"])
        kw["angles"] = dict(i=t[:, 0], j=t[:, 1], k=t[:, 2], kth=r32(rng.uniform(300, 600, len(t))), th0=r32(rng.uniform(1.6, 2.2, len(t))))
    if terms["torsions"]:
        t = np.array(terms["torsions"])
        kw["torsions"] = dict(i=t[:, 0], j=t[:, 1], k=t[:, 2], l=t[:, 3], periodicity=rng.integers(1, 7, len(t)), phase=r32(rng.uniform(-math.pi, math.pi, len(t))),
                              k0=r32(rng.uniform(0.5, 5.0, len(t))))
    if terms["excl"]:
        kw["ewald_excl"] = np.array(terms["excl"]); kw["excluded"] = np.array(terms["excl"])
    case = S.Case(x, 8.0, coul=dict(kind="ewald", rc=1.0), r_list=1.2, charge=r32(rng.normal(size=n) * 0.4), mass=np.full(n, 12.0), velocities=np.zeros((n, 3)),
                  lj=dict(cutoff=("distance", 1.0)) if lj else None, sigma=np.full(n, 0.05) if lj else None, eps=np.full(n, 0.5) if lj else None, name=f"hub{m}", **kw)
    case.slots = slot_counts(case)
    case.n_with_terms = n_with
    assert case.slots[0] == m and (case.slots[n_with:] == 0).all() and (case.slots[:n_with] > 0).all()
    return case


def slot_counts(case):
    """per atom, the number of term slots it takes part in"""
    slots = np.zeros(case.n, np.int64)
    for d, roles in ((case.bonds, "ij"), (case.angles, "ijk"), (case.torsions, "ijkl")):
        if d is not None:
            for r in roles: np.add.at(slots, np.asarray(d[r], dtype=np.int64), 1)
    if case.ewald_excl is not None:
        np.add.at(slots, np.asarray(case.ewald_excl, dtype=np.int64).reshape(-1), 1)
    return slots


def permuted(case, seed=0):
    """the coordinates of `case` (from chains(): equal-length chains) handed round among the chains by a random permutation without fixed points: every term now
    joins atoms whose indices sit in one chain and whose coordinates sit where another chain was, bonded partners still next to each other"""
    rng = np.random.default_rng([seed, 77])
    topo = case.topo_chains
    while True:
        p = rng.permutation(len(topo))
        if not np.any(p == np.arange(len(topo))):
            break
    x = case.coords.copy()
    for dst, src in enumerate(p):
        x[topo[dst]] = case.coords[topo[src]]
    return x


# ---- degenerate and near-degenerate geometry: every coordinate is exactly representable in fp32 (multiples of 1/64 nm, or a small fp32 number next to a face) ----
U = 1.0 / 64.0


def _f32(v):
    return float(np.float32(v))


def _case(x, name, charge=None, **kw):
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), "coordinates must be exact in fp32"
    n = len(x)
    return S.Case(x, 8.0, coul=dict(kind="ewald", rc=1.0), r_list=1.2, charge=np.zeros(n) if charge is None else np.asarray(charge, dtype=np.float64),
                  mass=np.full(n, 12.0), velocities=np.zeros((n, 3)), name=name, **kw)


def collinear_angles(bent=False):
    """two axis-aligned angles, straight (θ = π) and folded (θ = 0); bent=True: the same atoms with the end atoms moved off the axis (the geometry evaluated first
    in the stale-slot check).  θ0 = 1.75, kθ = 384 (exact in fp32)."""
    dy = 8 * U if bent else 0.0
    x = [[64 * U, 64 * U, 64 * U], [72 * U, 64 * U, 64 * U], [80 * U, 64 * U + dy, 64 * U],          # i – j – k along x
         [136 * U, 64 * U + dy, 128 * U], [128 * U, 64 * U, 128 * U], [144 * U, 64 * U, 128 * U]]     # j at the end: both arms point the same way
    a = dict(i=[0, 3], j=[1, 4], k=[2, 5], kth=[384.0, 384.0], th0=[1.75, 1.75])
    return _case(x, "collinear_bent" if bent else "collinear", angles={k: np.array(v) for k, v in a.items()})


def near_collinear_angles(delta):
    """angles `delta` rad off straight and off folded, four arm lengths each: the off-axis offset is a small fp32 number next to the y = 0 face.  The first arm is 8/64
    nm; the second is never that long: a folded angle with equal arms is mirror-symmetric, the two end forces cancel on the middle atom INSIDE the term (to δ of
    their size), and S_i — the norm of the term's net force on the atom — no longer says how large the numbers are that were added."""
    x, ai = [], []
    for q, arm in enumerate((6, 9, 11, 13)):
        for folded in (False, True):
            base = np.array([(32 + 48 * q) * U, 0.0, (64 + 64 * folded) * U])
            j = base; i = base + np.array([8 * U, 0, 0])
            sgn = 1.0 if folded else -1.0
            k = base + np.array([sgn * arm * U, _f32(arm * U * math.tan(delta)), 0.0])
            n0 = len(x); x += [i, j, k]; ai.append((n0, n0 + 1, n0 + 2))
    t = np.array(ai)
    return _case(x, f"near_collinear_{delta:g}", angles=dict(i=t[:, 0], j=t[:, 1], k=t[:, 2], kth=np.full(len(t), 384.0), th0=np.full(len(t), 1.75)))


def planar_torsions(delta=0.0):
    """torsions with periodicities 1–6 and phases 0 and π (as fp32 holds it).  delta = 0: exactly planar, cis and trans, in a z = const plane.  delta > 0: `delta` rad on
    either side of ±π (the last atom lifted off the z = 0 plane, or the other three), three arm lengths each, k0 = 2.5 on one side and 1.5 on the other (so that the two
    sides' virials do not cancel)."""
    x, tt, per, ph, k0 = [], [], [], [], []
    slot = 0
    geoms = (("cis", 8), ("trans", 8)) if delta == 0.0 else tuple((side, arm) for side in ("+", "-") for arm in (7, 8, 11))
    for n in range(1, 7):
        for phase in (0.0, _f32(math.pi)):
            for g, arm in geoms:
                bx, by = (16 + 40 * (slot % 12)) * U, (16 + 40 * (slot // 12)) * U; slot += 1
                z = 64 * U if delta == 0.0 else 0.0
                i = [bx, by + 8 * U, z]; j = [bx, by, z]; k = [bx + 8 * U, by, z]
                l = [bx + 8 * U, by + (arm if g == "cis" else -arm) * U, z]
                if g == "+": l[2] = _f32(arm * U * math.tan(delta))
                if g == "-": i[2] = j[2] = k[2] = _f32(arm * U * math.tan(delta))
                n0 = len(x); x += [i, j, k, l]; tt.append((n0, n0 + 1, n0 + 2, n0 + 3)); per.append(n); ph.append(phase); k0.append(1.5 if g == "-" else 2.5)
    t = np.array(tt)
    assert slot <= 144
    return _case(x, f"planar_torsions_{delta:g}", torsions=dict(i=t[:, 0], j=t[:, 1], k=t[:, 2], l=t[:, 3], periodicity=np.array(per), phase=np.array(ph),
                                                              k0=np.array(k0)))


def torsion_angles(case):
    """φ of every torsion of a case (float64, the definition of Ref.term_energies)"""
    r = Ref(case, np.float64); p = r.x[r.idx["torsions"]]
    ab, bc, cd = (r.image(p[:, q + 1] - p[:, q], r.basis) for q in range(3))
    n1, n2 = np.cross(ab, bc), np.cross(bc, cd)
    return np.arctan2((np.cross(n1, n2) * bc).sum(axis=1) / np.linalg.norm(bc, axis=1), (n1 * n2).sum(axis=1))


def exclusion_pairs(coincident=False):
    """Ewald exclusion pairs: separations 1/64 nm and 1.0 nm (along x, y, z and a diagonal), and pairs with one charge zero.  coincident=True: pairs of atoms on
    the same point instead (erf(αr) = 0 ≤ 1e-6: the zero-force path, the limit energy −2α·ke·qi·qj/√π)."""
    x, e, q = [], [], []
    if coincident:
        for p in ([64 * U, 64 * U, 64 * U], [0.0, 128 * U, 511 * U]):
            n0 = len(x); x += [p, p]; e.append((n0, n0 + 1)); q += [0.5, -0.75]
        return _case(x, "excl_coincident", charge=q, ewald_excl=np.array(e), excluded=np.array(e))
    slot = 0
    for sep in (U, 64 * U):
        for d in ([1, 0, 0], [0, 1, 0], [0, 0, 1]):
            for qq in ((0.5, -0.75), (0.5, 0.0)):
                a = np.array([(32 + 8 * slot) * U, (32 + 8 * slot) * U, 96 * U]); slot += 1
                n0 = len(x); x += [a, a + sep * np.array(d, dtype=np.float64)]; e.append((n0, n0 + 1)); q += list(qq)
    for qq in ((0.625, 0.375),):      # a diagonal: 1/64 along every axis
        a = np.array([300 * U, 20 * U, 30 * U]); n0 = len(x); x += [a, a + U]; e.append((n0, n0 + 1)); q += list(qq)
    return _case(x, "excl_pairs", charge=q, ewald_excl=np.array(e), excluded=np.array(e))


def face_bonds():
    """bonds across each periodic face of the 8 nm box, atoms at 1/64 and L − 1/64 (r = 1/32 through the face), in both orders; and a bond with r = r0 exactly"""
    L = 8.0
    x, b, r0 = [], [], []
    for d in range(3):
        for flip in (False, True):
            lo = np.array([(100 + 10 * d) * U, (200 + 10 * d) * U, (300 + 10 * d) * U]); hi = lo.copy()
            lo[d] = U; hi[d] = L - U
            n0 = len(x); x += [hi, lo] if flip else [lo, hi]; b.append((n0, n0 + 1)); r0.append(0.125)
    t = np.array(b)
    return _case(x, "face_bonds", bonds=dict(i=t[:, 0], j=t[:, 1], k=np.full(len(t), 262144.0), r0=np.array(r0)))


def exact_bond():
    """a bond with r = r0 = 1/8 nm exactly, along y: energy and forces are exactly zero in every precision"""
    return _case([[64 * U, 64 * U, 64 * U], [64 * U, 72 * U, 64 * U]], "exact_bond", bonds=dict(i=np.array([0]), j=np.array([1]), k=np.array([262144.0]), r0=np.array([0.125])))


def full_scale_torsions(case):
    """a twin of a torsion case with periodicity 1 and phase π/2 throughout: there dE/dφ = ±k at φ = 0 and ±π, so n times the twin's per-atom scale is the size a
    torsion force can have at that geometry — the yardstick where the force itself vanishes (planar torsions with phase 0 or π: sin(nφ − phase) = 0)"""
    import copy
    twin = copy.copy(case)
    t = dict(case.torsions); n = np.asarray(t["periodicity"], dtype=np.float64)
    t["periodicity"] = np.ones(len(n), dtype=np.int64); t["phase"] = np.full(len(n), math.pi / 2)
    twin.torsions = t
    r = Ref(twin, np.longdouble)
    s = np.zeros(case.n)
    for q in range(4):
        np.add.at(s, r.idx["torsions"][:, q], n * np.asarray(np.sqrt((r.term_forces()["torsions"][:, q] ** 2).sum(axis=1)), dtype=np.float64))
    return s


# ---- what the fp32 bars are made of -------------------------------------------------------------------------------
def compare(f, e, w, f_ref, e_ref, w_ref, scale, wscale=None):
    """(worst per-atom ‖Δf_i‖ / S_i over the atoms with S_i > 0, |ΔE| / |E|, max |ΔW| / max |W| (or / wscale, where given), number of atoms compared)"""
    m = scale > 0
    df = np.linalg.norm(np.asarray(f, dtype=np.float64) - np.asarray(f_ref, dtype=np.float64), axis=1)
    rf = float((df[m] / scale[m]).max()) if m.any() else 0.0
    re = abs(float(e) - float(e_ref)) / abs(float(e_ref)) if float(e_ref) != 0.0 else abs(float(e))
    w, w_ref = np.asarray(w, dtype=np.float64), np.asarray(w_ref, dtype=np.float64)
    wmax = float(np.abs(w_ref).max()) if wscale is None else float(wscale)
    rw = float(np.abs(w - w_ref).max() / wmax) if wmax > 0 else float(np.abs(w).max())
    return rf, re, rw, int(m.sum())


def oracle_all(case, dtype, coords=None):
    o = case.oracle(dtype, coords=coords)
    return (o.forces(None, pairwise=False, specific=True).astype(np.float64), o.potential_energy(None, pairwise=False, specific=True),
            o.virial(None, pairwise=False, specific=True))


def fp32_yardstick(case, coords=None, scale=None, wscale=None):
    """the oracle's own arithmetic in fp32 (correctly rounded host libm) against itself in fp64 on the same inputs: compare()'s three ratios"""
    import copy
    if coords is not None:
        case = copy.copy(case); case.coords = np.asarray(coords, dtype=np.float64)
    scale = per_atom_scale(case) if scale is None else scale
    return compare(*oracle_all(case, np.float32), *oracle_all(case, np.float64), scale, wscale)[:3]


COUNTS = (1, 63, 64, 65, 129)
HUB_M = (7, 8, 9, 31, 32, 33, 64, 65, 100)
HUB_M_MIXED = (7, 8, 9, 11) + HUB_M[3:]      # 11: the fewest slots with the hub in every role of every type
KW = dict(bonds="n_bonds", angles="n_angles", torsions="n_torsions", excl="n_excl")


def mixed_cases(seed=0):
    """every present type with n ≡ 1 (mod 64); bonds and torsions only (an empty range in the middle and at the end)"""
    return [chains(n_bonds=65, n_angles=129, n_torsions=1, n_excl=65, seed=seed), chains(n_bonds=65, n_torsions=129, seed=seed)]


def regular_groups(seed=0):
    """{group: [cases]} of the regular systems of tests/test_gpu_bonded.py for one seed (the bead chain has no seed: it is one system)"""
    g = {f"a_{ty}": [chains(seed=seed, **{KW[ty]: n}) for n in COUNTS] for ty in TYPES}
    g["a_mixed"] = mixed_cases(seed)
    g["hub_bonds"] = [hub(m, False, seed) for m in HUB_M]
    g["hub_mixed"] = [hub(m, True, seed) for m in HUB_M_MIXED]
    c = chains(40, 40, 40, 40, seed=seed); c.coords = permuted(c, seed)
    g["resort"] = [c]
    g["tri"] = [chains(65, 65, 65, 65, seed=seed, triclinic=True)]
    if seed == 0:
        b = bead_chain()
        g["bead_all"] = [b]
        for ty in TYPES: g[f"bead_{ty}"] = [only(b, ty)]
    return g


def degenerate_groups():
    return {"near_collinear_1e-3": [near_collinear_angles(1e-3)], "near_collinear_1e-5": [near_collinear_angles(1e-5)], "torsion_planar": [planar_torsions(0.0)],
            "torsion_near_pi": [planar_torsions(1e-4)], "excl_pairs": [exclusion_pairs()], "face_bonds": [face_bonds()]}


def group_step(group):
    return H_NEAR if group.startswith("near_collinear") else H_FD


def group_scale(group, case):
    """the per-atom scale a group's force errors are measured against: S_i, except for the exactly planar torsions (full_scale_torsions)"""
    return full_scale_torsions(case) if group == "torsion_planar" else per_atom_scale(case, h=group_step(group))


def ref_all(group, case):
    """forces, energy and virial of a case by the longdouble reference, as float64"""
    r = of_case(case, np.longdouble); h = group_step(group)
    return np.asarray(r.forces(h=h), dtype=np.float64), float(r.energy()), np.asarray(r.virial(h=h), dtype=np.float64)


def group_wscale(group, case):
    """what a group's virial errors are measured against: None = the largest component of the reference tensor (the regular systems and most others); the
    planar-torsion and the near-collinear groups, whose tensor all but vanishes next to the forces it is made of, take Ref.virial_scale"""
    if group == "torsion_planar":
        import copy
        twin = copy.copy(case); t = dict(case.torsions); t["periodicity"] = np.ones(len(t["i"]), dtype=np.int64); t["phase"] = np.full(len(t["i"]), math.pi / 2); twin.torsions = t
        return 6.0 * of_case(twin).virial_scale()
    if group == "torsion_near_pi" or group.startswith("near_collinear"):      # (θ is stationary under a strain at θ = 0 and π: an angle's virial goes with sin θ)
        return of_case(case).virial_scale(h=group_step(group))
    return None


def oracle_vs_ref(group, case, scale=None):
    """the fp64 oracle against the longdouble reference: compare()'s three ratios (the oracle's virial is symmetric to rounding; its symmetric part is compared)"""
    f, e, w = oracle_all(case, np.float64)
    scale = group_scale(group, case) if scale is None else scale
    return compare(f, e, 0.5 * (w + w.T), *ref_all(group, case), scale, group_wscale(group, case))[:3]


def nondifferentiable_terms(case):
    """the terms whose energy has no derivative where they stand — an EXACTLY collinear angle (θ = 0 or π: the energy has a cone there) and an exclusion pair at
    r = 0 (the force's direction is undefined) — as {type: indices}.  The finite-difference reference is not asked about these, and about nothing else."""
    r = Ref(case, np.float64)
    out = {}
    if "angles" in r.idx:
        p = r.x[r.idx["angles"]]
        c = np.cross(r.image(p[:, 0] - p[:, 1], r.basis), r.image(p[:, 2] - p[:, 1], r.basis))
        if np.any(np.all(c == 0.0, axis=1)): out["angles"] = np.nonzero(np.all(c == 0.0, axis=1))[0]
    if "excl" in r.idx:
        p = r.x[r.idx["excl"]]
        d = r.image(p[:, 1] - p[:, 0], r.basis)
        if np.any(np.all(d == 0.0, axis=1)): out["excl"] = np.nonzero(np.all(d == 0.0, axis=1))[0]
    return out


# ---- the launch shapes of a run: chains in a small fluid ---------------------------------------------------------------
RUN_DT = 0.0005


def fluid_with_chains(kind, seed=0, n_side=12):
    """S.lj_fluid(n_side) (argon, fp32 coordinates) with chains of 70 bonds, 65 angles and 130 torsion entries added as further atoms: 2 + 2 + 3 = 7 term blocks of 64
    lanes — not a multiple of four, and no exclusion terms, so a launch that rounds the block count up to whole 256-lane workgroups has an idle term block, which
    lands in the exclusion branch with null arrays.  The chain atoms carry charges (zero in sum), no LJ well (ϵ = 0: they may sit anywhere in the fluid) and have
    their 1-2 and 1-3 pairs excluded from the pair list.  kind "rf": CoulombReactionField; "pme": CoulombEwald + PME.  At rest."""
    fl = S.lj_fluid(n_side, dtype=np.float32)
    ch = chains(n_bonds=70, n_angles=65, n_torsions=130, seed=seed, box=float(fl.box[0]))
    n0, n1 = fl.n, ch.n
    off = lambda d, keys: {k: (np.asarray(v) + n0 if k in keys else np.asarray(v)) for k, v in d.items()}
    excl = np.concatenate([np.stack([c[:-1], c[1:]], 1) for c in ch.topo_chains] + [np.stack([c[:-2], c[2:]], 1) for c in ch.topo_chains]) + n0
    q = np.concatenate([np.zeros(n0), ch.charge - ch.charge.mean()]).astype(np.float32).astype(np.float64)
    coul = dict(kind="rf", rc=1.0) if kind == "rf" else dict(kind="ewald", rc=1.0)
    case = S.Case(np.concatenate([fl.coords, ch.coords]), fl.box, lj=dict(cutoff=("distance", 1.0)), coul=coul, r_list=1.2, rebuild_every=10,
                  velocities=np.zeros((n0 + n1, 3)), charge=q, sigma=np.concatenate([fl.sigma, np.full(n1, 0.2)]), eps=np.concatenate([fl.eps, np.zeros(n1)]),
                  mass=np.concatenate([fl.mass, np.full(n1, 12.0)]), excluded=excl, bonds=off(ch.bonds, "ij"), angles=off(ch.angles, "ijk"),
                  torsions=off(ch.torsions, "ijkl"), pme=dict(order=5) if kind == "pme" else None, name=f"fluid_chains_{kind}")
    case.n_fluid = n0
    nt = n_terms(case)
    assert nt["excl"] == 0 and sum(-(-nt[t] // 64) for t in TYPES) % 4 != 0
    return case


def velocity_scale(case, n_steps, dt=RUN_DT):
    """V_i = n·dt/m_i · (S_i + Σ_j‖f_ij‖) at the starting coordinates: from rest, v_i after n steps is a sum of n forces times dt/m_i (half weights at the ends),
    so V_i is the size of what has been summed into it"""
    o = case.oracle(np.float64)
    pair, _ = o.force_scale(o.neighbors("cell"))
    return n_steps * dt / case.mass * (per_atom_scale(case) + pair)


def oracle_run(case, dtype, n_steps, dt=RUN_DT):
    o = case.oracle(dtype)
    o.vv_run(n_steps, dt, remove_cm_every=1, nthreads=4, specific=True, general=case.pme is not None)
    return np.asarray(o.vel, dtype=np.float64)
