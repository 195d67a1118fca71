"""Exception lists (excluded / special pairs) of the neighbour search: test systems, topology generators and a plain numpy reference.

The reference is a brute force over all pairs in fp64 (minimum image; the nearest of the 27 neighbouring images in a triclinic cell) that knows
nothing of the engine or of the C++ oracle: it normalises the two raw pair lists itself (a pair in both is excluded, duplicates and reversed order
collapse, i == j and indices outside [0, n) are invalid), decides each pair (plain / special / excluded) and evaluates LJ + Coulomb (plain with a
distance cutoff, or reaction field) per pair.  It returns the DIRECTED full list — for every atom its partners and their flags — because the search
kernel takes its verdicts per directed view: the view of the lower-indexed atom (caller-index offset δ > 0) and the view of the higher one (δ < 0)
come from different mask words, and only the first shows in an exported list.  tests/test_exceptions_host.py checks this reference against the
oracle; tests/test_gpu_exceptions.py checks the engine against it."""
import functools
import math

import numpy as np

from tests import systems as S

KE = 138.93545764          # kJ mol⁻¹ nm e⁻² (the Coulomb constant of Molly and of include/mollyhip.h)
PLAIN, SPECIAL, EXCLUDED = 0, 1, 2
MIN_DIST = 0.27
VISIBLE = 20.0             # every pair inside the cutoff: half its force >= VISIBLE x the force bar of both its atoms
RF_DIELECTRIC = 4.0        # of the reaction-field cases: the force at the cutoff stays a third of the bare Coulomb force.  With 78.3 it all but vanishes there and
                           # 3.6 % of the pairs inside the cutoff of the base gas fall below VISIBLE bars (measured), over the 1 % that such a system may have
BAND = 1e-5                # |r²/r_list² − 1| below which the list decision is repeated in the precision under test


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------------
def _vector_1d(c1, c2, L):
    """spatial.jl:491-500 vector_1D in the arrays' own precision: compare / select, not v − L·round(v / L)"""
    v = c2 - c1
    vp, vm = v + L, v - L
    return np.where(v > 0, np.where(v < -vm, v, vm), np.where(-v < vp, v, vp))


def _displacements(c1, c2, box, basis):
    """minimum-image vectors c2 − c1 of broadcastable (…, 3) arrays, in the precision of the inputs"""
    T = c1.dtype
    if basis is None:
        return np.stack([_vector_1d(c1[..., d], c2[..., d], T.type(box[d])) for d in range(3)], -1)
    bv = np.asarray(basis, dtype=T)
    shape = np.broadcast_shapes(c1.shape, c2.shape)
    best = np.full(shape[:-1], np.inf, T)
    out = np.zeros(shape, T)
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):      # spatial.jl:536-551: the first minimum in this loop order
                e = np.broadcast_to((((c2 + T.type(ox) * bv[0]) + T.type(oy) * bv[1]) + T.type(oz) * bv[2]) - c1, shape)
                sq = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                m = sq < best
                best = np.where(m, sq, best)
                out[m] = e[m]
    return out


def _norm2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def all_pairs_within(coords, box, r, basis=None, dtype=np.float64, chunk=256):
    """every pair lo < hi with |x_hi − x_lo| <= r, the decision taken in `dtype` arithmetic: (lo, hi, dr fp64 from lo to hi).  The fp64 pass finds
    the candidates; the few within BAND of r are decided again in fp32 when that is the precision under test.  In a triclinic cell the 27-image
    search runs on the pairs that pass a necessary condition: a vector no longer than r has a component of at most r / h_k along the k-th
    reciprocal axis (h_k the cell's height), which is its fractional coordinate difference, wrapped — exact while r < h_k / 2."""
    x = np.ascontiguousarray(coords, dtype=np.float64)
    n = len(x)
    sq = np.float64(r) * np.float64(r)
    lo, hi, dr = [], [], []
    if basis is not None:
        inv = np.linalg.inv(np.asarray(basis, dtype=np.float64))      # rows of `basis` are the cell vectors: frac = x @ inv
        reach = r * (1.0 + 1e-6) * np.linalg.norm(inv, axis=0)          # r / h_k
        assert reach.max() < 0.5
        fr = x @ inv
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        upper = np.arange(n)[None, :] > np.arange(a, b)[:, None]
        if basis is None:
            d = _displacements(x[a:b, None, :], x[None, :, :], box, basis)
            ii, jj = np.nonzero((_norm2(d) <= sq * (1.0 + BAND)) & upper)
            d = d[ii, jj]
        else:
            df = fr[None, :, :] - fr[a:b, None, :]
            df -= np.round(df)
            ii, jj = np.nonzero((np.abs(df) <= reach).all(axis=-1) & upper)
            d = _displacements(x[a + ii], x[jj], box, basis)
            m = _norm2(d) <= sq * (1.0 + BAND)
            ii, jj, d = ii[m], jj[m], d[m]
        r2 = _norm2(d)
        keep = r2 <= sq
        if np.dtype(dtype) == np.float32:
            x32 = x.astype(np.float32)
            for k in np.nonzero(np.abs(r2 / sq - 1.0) <= BAND)[0]:
                # neighbors.jl:404-412 takes vector(coords[i], coords[j]) with i > j
                d32 = _displacements(x32[jj[k]], x32[a + ii[k]], box, basis)
                keep[k] = _norm2(d32) <= np.float32(r) * np.float32(r)
        lo.append(a + ii[keep]); hi.append(jj[keep]); dr.append(d[keep])
    return np.concatenate(lo).astype(np.int64), np.concatenate(hi).astype(np.int64), np.concatenate(dr)


# ---- normalisation of raw exception lists -------------------------------------------------------------------------------------------------------
def normalise(n, excluded, special):
    """raw (m, 2) lists in any order, with duplicates → {(lo, hi): EXCLUDED | SPECIAL}; ValueError for i == j or an index outside [0, n)"""
    out = {}
    for pairs, kind in ((special, SPECIAL), (excluded, EXCLUDED)):      # excluded last: it wins
        for i, j in ([] if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()):
            if i == j or not (0 <= i < n and 0 <= j < n):
                raise ValueError(f"invalid exception pair ({i}, {j}) for {n} atoms")
            out[(min(i, j), max(i, j))] = kind
    return out


# ---- per-pair physics ---------------------------------------------------------------------------------------------------------------------------
def _pair_terms(case, r, qq, sig, eps, special):
    """radial force (positive: repulsive) and energy of pairs at distance r with q_i q_j, mixed σ, ϵ — the flag `special` for all of them"""
    f = np.zeros_like(r); e = np.zeros_like(r)
    if case.lj is not None:
        kind, rc = case.lj["cutoff"][0], case.lj["cutoff"][1]
        assert kind == "distance"
        w = case.lj.get("weight_special", 1.0) if special else 1.0
        six = (sig * sig / (r * r)) ** 3
        on = (r <= rc) & (eps > 0) & (sig > 0)
        f += np.where(on, w * (24.0 * eps / r) * (2.0 * six * six - six), 0.0)
        e += np.where(on, w * 4.0 * eps * (six * six - six), 0.0)
    if case.coul is not None:
        w = case.coul.get("weight_special", 1.0) if special else 1.0
        if case.coul["kind"] == "plain":
            kind, rc = case.coul["cutoff"][0], case.coul["cutoff"][1]
            assert kind == "distance"
            on = r <= rc
            f += np.where(on, w * KE * qq / (r * r), 0.0)
            e += np.where(on, w * KE * qq / r, 0.0)
        else:
            assert case.coul["kind"] == "rf"
            rc, erf = case.coul["rc"], case.coul.get("eps_rf", 78.3)
            krf = 0.0 if special else ((1.0 / (2.0 * rc ** 3)) if math.isinf(erf) else (erf - 1.0) / ((2.0 * erf + 1.0) * rc ** 3))
            crf = 0.0 if special else ((1.5 / rc) if math.isinf(erf) else 3.0 * erf / ((2.0 * erf + 1.0) * rc))
            on = r <= rc
            f += np.where(on, w * KE * qq * (1.0 / (r * r) - 2.0 * krf * r), 0.0)
            e += np.where(on, w * KE * qq * (1.0 / r + krf * r * r - crf), 0.0)
    return f, e


def interaction_cutoff(case):
    rc = 0.0
    if case.lj is not None: rc = max(rc, case.lj["cutoff"][1])
    if case.coul is not None: rc = max(rc, case.coul["cutoff"][1] if case.coul["kind"] == "plain" else case.coul["rc"])
    return rc


class Reference:
    """All pairs within r_list of a case, each with its verdict and its force and energy as a plain and as a special pair"""

    def __init__(self, case, dtype=np.float64, coords=None, excluded="case", special="case", geometry=None):
        self.case, self.n = case, case.n
        x = np.asarray(case.coords if coords is None else coords, dtype=np.float64)
        basis = None if case.triclinic is None else np.asarray(case.triclinic["basis"], dtype=np.float64)
        assert basis is None or not case.triclinic.get("approx_images", True), "the reference takes the nearest of 27 images"
        # geometry: the pairs of another reference on the same coordinates, box, r_list and precision (the brute force is the expensive part)
        self.lo, self.hi, self.dr = geometry if geometry is not None else all_pairs_within(x, case.box, case.r_list, basis, dtype)
        self.geometry = (self.lo, self.hi, self.dr)
        self.r = np.sqrt((self.dr ** 2).sum(axis=1))
        self.exceptions = normalise(self.n, case.excluded if isinstance(excluded, str) else excluded, case.special if isinstance(special, str) else special)
        self.kind = np.array([self.exceptions.get(p, PLAIN) for p in zip(self.lo.tolist(), self.hi.tolist())], dtype=np.int8).reshape(-1)
        q = np.zeros(self.n) if case.charge is None else np.asarray(case.charge, dtype=np.float64)
        sg, ep = np.asarray(case.sigma, dtype=np.float64), np.asarray(case.eps, dtype=np.float64)
        qq, sig, eps = q[self.lo] * q[self.hi], 0.5 * (sg[self.lo] + sg[self.hi]), np.sqrt(ep[self.lo] * ep[self.hi])
        self.f_plain, self.e_plain = _pair_terms(case, self.r, qq, sig, eps, False)
        self.f_special, self.e_special = _pair_terms(case, self.r, qq, sig, eps, True)
        self.rc = interaction_cutoff(case)
        self.f_pair = np.where(self.kind == PLAIN, self.f_plain, np.where(self.kind == SPECIAL, self.f_special, 0.0))     # signed radial force of the chosen interaction
        self.e_pair = np.where(self.kind == PLAIN, self.e_plain, np.where(self.kind == SPECIAL, self.e_special, 0.0))
        self.unit = self.dr / self.r[:, None]

    # -- lists --
    def half_list(self):
        """(lo, hi, special) of the list pairs, sorted as systems.sorted_pairs sorts"""
        m = self.kind != EXCLUDED
        return S.sorted_pairs(self.lo[m], self.hi[m], (self.kind[m] == SPECIAL).astype(np.uint8))

    def directed(self):
        """the full list as the force kernels walk it: (atom, partner, special flag, |f| of the chosen interaction), sorted by atom, then partner"""
        m = self.kind != EXCLUDED
        a = np.concatenate([self.lo[m], self.hi[m]]); b = np.concatenate([self.hi[m], self.lo[m]])
        sp = np.tile((self.kind[m] == SPECIAL).astype(np.uint8), 2); f = np.tile(np.abs(self.f_pair[m]), 2)
        o = np.lexsort((b, a))
        return a[o], b[o], sp[o], f[o]

    # -- sums --
    def forces(self):
        f = np.zeros((self.n, 3))
        v = self.f_pair[:, None] * self.unit          # on hi; the opposite on lo
        np.add.at(f, self.hi, v); np.add.at(f, self.lo, -v)
        return f

    def potential_energy(self):
        return float(self.e_pair.sum())

    def force_scale(self):
        """Σ_j |f_ij| per atom over the list"""
        s = np.zeros(self.n)
        np.add.at(s, self.lo, np.abs(self.f_pair)); np.add.at(s, self.hi, np.abs(self.f_pair))
        return s

    def cutoff_jump(self, rel_band=2e-6):
        """per atom, the force of pairs within rel_band of the hard cutoff, where fp32 may take `r <= rc` the other way (systems.fp32_force_tolerance)"""
        j = np.zeros(self.n)
        m = (np.abs(self.r / self.rc - 1.0) <= rel_band) & (self.kind != EXCLUDED)
        fj = np.maximum(np.abs(self.f_plain), np.abs(self.f_special))[m]
        np.add.at(j, self.lo[m], fj); np.add.at(j, self.hi[m], fj)
        return j

    def bar(self, dtype, jumps=True):
        """the per-atom force bar: fp32 4e-5·Σ_j|f_ij| + 1e-6, the project's (systems.fp32_force_tolerance, which also allows the force of a pair within
        2e-6 of the hard cutoff to come or go: jumps); fp64 rtol 1e-8, atol 1e-9 as test_exclusions_and_special_pairs has them"""
        if np.dtype(dtype) == np.float32:
            return 4e-5 * self.force_scale() + (1.01 * self.cutoff_jump() if jumps else 0.0) + 1e-6
        return 1e-9 + 1e-8 * np.linalg.norm(self.forces(), axis=1)

    def inside(self):
        """the list pairs that interact: inside the cutoff and not excluded"""
        return (self.r <= self.rc) & (self.kind != EXCLUDED)

    def visibility(self, dtype):
        """per interacting pair: 0.5·|f_ij| over the larger of its two atoms' bars"""
        m = self.inside()
        bar = self.bar(dtype, jumps=False)
        return 0.5 * np.abs(self.f_pair[m]) / np.maximum(bar[self.lo[m]], bar[self.hi[m]])

    def wrong_verdict_effect(self):
        """per pair within r_list, the smallest force change that a wrong verdict on it causes (a flag flip, a dropped or a resurrected entry) — for
        the excepted pairs, where a wrong verdict may also be `plain` instead of `excluded`"""
        fp, fs = np.abs(self.f_plain), np.abs(self.f_special)
        return np.where(self.kind == PLAIN, np.minimum(fp, np.abs(fp - fs)), np.where(self.kind == SPECIAL, np.minimum(fs, np.abs(fp - fs)), np.minimum(fp, fs)))

    def explain(self, atom, df, tol):
        """which single wrong directed entry of `atom` explains the force difference df (3-vector, engine − reference)?  → text"""
        m = (self.lo == atom) | (self.hi == atom)
        out = []
        for k in np.nonzero(m)[0]:
            other = int(self.hi[k] if self.lo[k] == atom else self.lo[k])
            u = self.unit[k] * (1.0 if self.hi[k] == atom else -1.0)          # direction of a repulsive force on `atom`
            have = self.f_pair[k]
            for name, f in (("plain", self.f_plain[k]), ("special", self.f_special[k]), ("excluded/missing", 0.0)):
                if f == have: continue
                res = np.linalg.norm(df - (f - have) * u)
                if res <= max(tol, 1e-3 * np.linalg.norm(df)):
                    out.append(f"partner {other} (caller offset δ = {other - atom:+d}, r = {self.r[k]:.4f}, should be {('plain', 'special', 'excluded')[self.kind[k]]}) was taken as {name}")
        exc = sorted(b - atom if a == atom else a - atom for (a, b) in self.exceptions if atom in (a, b))
        return f"atom {atom}, |Δf| = {np.linalg.norm(df):.4g}, offsets to its excepted partners {exc}: " + ("; ".join(out) if out else "no single entry explains it")


# ---- systems ------------------------------------------------------------------------------------------------------------------------------------
def _place(rng, n, box, basis, have, dmin, sphere=None):
    """random sequential placement of n points at least dmin (minimum image) from each other and from `have`"""
    pts = [np.asarray(p) for p in have]
    new = []
    bv = np.diag(box) if basis is None else np.asarray(basis)
    inv = np.linalg.inv(bv); reach = dmin * (1.0 + 1e-6) * np.linalg.norm(inv, axis=0)
    tries = 0
    while len(new) < n:
        tries += 1
        assert tries < 400 * n + 10000, "placement jammed"
        if sphere is None:
            p = rng.random(3) @ bv
        else:
            c, rad = sphere
            p = rng.normal(size=3); p = c + p / np.linalg.norm(p) * rad * rng.random() ** (1.0 / 3.0)
        if pts:
            X = np.asarray(pts)
            if basis is None:
                d = X - p; d -= np.round(d / box) * box
                ok = (d * d).sum(axis=1).min() >= dmin * dmin
            else:      # the 27-image search only for the points that can be that close (see all_pairs_within)
                df = (X - p) @ inv; df -= np.round(df)
                X = X[(np.abs(df) <= reach).all(axis=1)]
                ok = len(X) == 0 or _norm2(_displacements(p[None, :], X, box, basis)).min() >= dmin * dmin
            if not ok: continue
        pts.append(p); new.append(p)
    return np.asarray(new)


def _wrap(x, box, basis):
    if basis is None:
        x = x - np.floor(x / box) * box
        return np.where(x >= box, 0.0, x)
    fr = np.linalg.solve(np.asarray(basis).T, x.T).T
    fr -= np.floor(fr)
    return fr @ np.asarray(basis)


SYSTEMS = {   # name: n, box or basis, cutoff, r_list, blobs ((first caller index, atoms, radius), …), seed
    "gas1024": dict(n=1024, box=4.2, rc=0.75, r_list=0.8, seed=1, v=3.0),          # the base system
    # the coordinates of blobs1024 for the one-type LJ fluid.  σ 0.25 nm and a 0.6 nm cutoff: with σ 0.3 the contact pairs sit high on the repulsive wall (462 against 0.6
    # kJ/mol/nm at 0.6 nm) and 3.3 % of the pairs inside 0.6 nm fall below 20 bars; with σ 0.25 none does but the few at the zero crossing (0.2806 nm), measured
    "lj1024": dict(n=1024, box=4.2, rc=0.6, r_list=0.65, seed=2, sigma=0.25, blobs=((100, 40, 0.72), (300, 150, 1.12))),
    "blobs1024": dict(n=1024, box=4.2, rc=0.95, r_list=1.0, seed=2, blobs=((100, 40, 0.72), (300, 150, 1.12))),
    "gas2048": dict(n=2048, box=5.3, rc=0.75, r_list=0.8, seed=9),          # more than a few blocks at 256-atom blocks
    "small540": dict(n=540, box=3.4, rc=1.15, r_list=1.2, seed=4, blobs=((100, 40, 0.72), (300, 150, 1.12))),          # box < 2·(block half-extent + r_list): the in-loop exact minimum image
    "tri560": dict(n=560, basis=((3.45, 0, 0), (0.5, 3.35, 0), (-0.4, 0.6, 3.25)), rc=1.15, r_list=1.2, seed=5, blobs=((100, 40, 0.72), (300, 150, 1.12))),   # heights < 3 r_list: no cell grid
    "tri2048": dict(n=2048, basis=((5.4, 0, 0), (1.17, 5.22, 0), (-0.81, 1.35, 5.04)), rc=0.75, r_list=0.8, seed=6, blobs=((100, 40, 0.72), (300, 150, 1.12))),   # the sheared cell of test_gpu_triclinic, cut down
}


@functools.lru_cache(maxsize=None)
def _coordinates(name):
    p = SYSTEMS[name]
    rng = np.random.default_rng(p["seed"])
    basis = None if "basis" not in p else np.asarray(p["basis"], dtype=np.float64)
    box = np.full(3, p["box"]) if basis is None else np.diag(basis).copy()
    n = p["n"]
    x = np.zeros((n, 3)); taken = np.zeros(n, bool); have = []
    for k, (first, m, rad) in enumerate(p.get("blobs", ())):
        c = box * (0.27 + 0.46 * k)
        pts = _place(rng, m, box, basis, have, MIN_DIST, sphere=(c, rad))
        x[first:first + m] = pts; taken[first:first + m] = True; have += list(pts)
    x[~taken] = _place(rng, int((~taken).sum()), box, basis, have, MIN_DIST)
    x = _wrap(x, box, basis).astype(np.float32).astype(np.float64)      # one set of inputs for both precisions
    if basis is None: x = np.where(x >= np.float64(np.float32(box)), 0.0, x)
    x.setflags(write=False)
    return x, box, basis


def base_case(name, inter="coul", excluded=None, special=None):
    """The random gas `name` (caller order independent of position, minimum distance 0.27 nm, σ 0.3 nm unless the system names another, ϵ 1 kJ/mol).  inter: "coul" LJ + plain Coulomb with every
    charge +1 (the radial pair force is positive everywhere: no zero crossing), "lj" the one-type uncharged LJ fluid, "rf" LJ + reaction field, charges +1, σ 0.28 nm on the odd atoms.
    weight_special 0.5 for both interactions."""
    p = SYSTEMS[name]
    x, box, basis = _coordinates(name)
    n, rc = p["n"], p["rc"]
    rng = np.random.default_rng(p["seed"] + 100)
    # nm/ps, hot: in 30 steps of 0.5 fs the fastest atoms of a charged gas outrun the inner skin and the 0.2 nm outer margin — prunes, a second search — and every
    # pair still shows after the run.  2 nm/ps (0.145 nm) does that at r_list 1.0 nm; the base gas needs its 3 nm/ps (0.18 nm; 24 bars and more after the run), with
    # which the molecules of blobs1024 meet outsiders at 0.13 nm and a margin falls to 15.  The LJ fluid has no Coulomb repulsion to keep fast atoms apart: 0.6 nm/ps,
    # 0.03 nm in 20 steps, more than half its 0.05 nm skin
    v = rng.normal(size=(n, 3)) * (0.6 if inter == "lj" else p.get("v", 2.0))
    v -= v.mean(axis=0)
    sigma = np.full(n, p.get("sigma", 0.3))
    if inter == "rf": sigma[1::2] = 0.28      # two atom types: the group-split pass is for the general LJ kernels, not the one-type ones
    coul = {"coul": dict(kind="plain", cutoff=("distance", rc), weight_special=0.5), "rf": dict(kind="rf", rc=rc, eps_rf=RF_DIELECTRIC, weight_special=0.5), "lj": None}[inter]
    return S.Case(x, float(np.float32(box[0])) if basis is None else box, lj=dict(cutoff=("distance", rc), weight_special=0.5), coul=coul, r_list=p["r_list"], rebuild_every=10,
                  velocities=v.astype(np.float32).astype(np.float64), charge=None if inter == "lj" else np.ones(n), sigma=sigma, eps=np.full(n, 1.0),
                  mass=np.full(n, 39.948), excluded=excluded, special=special, triclinic=None if basis is None else dict(basis=basis, approx_images=False),
                  name=f"{name}_{inter}")


@functools.lru_cache(maxsize=None)
def _geometry(name, dtype_name):
    return Reference(base_case(name, "lj"), np.dtype(dtype_name)).geometry


@functools.lru_cache(maxsize=None)
def bare_reference(name, inter="coul"):
    """the reference of a system without any exception: what the topology generators choose their pairs from"""
    return Reference(base_case(name, inter), geometry=_geometry(name, "float64"))


# ---- topologies ---------------------------------------------------------------------------------------------------------------------------------
def excepted(ref, delta, count, min_visibility=None, dtype=np.float32, avoid=()):
    """up to `count` pairs inside the interaction cutoff at caller offset `delta`, alternately excluded and special → (excluded, special) lists of
    (lo, hi).  min_visibility: only pairs a wrong verdict on which moves a force by that many bars of both atoms (for interactions with a zero crossing)."""
    m = (ref.hi - ref.lo == delta) & (ref.r <= ref.rc)
    if min_visibility is not None:
        bar = ref.bar(dtype, jumps=False)
        m &= 0.5 * ref.wrong_verdict_effect() >= min_visibility * np.maximum(bar[ref.lo], bar[ref.hi])
    avoid = set(avoid)
    pairs = [(int(a), int(b)) for a, b in zip(ref.lo[m], ref.hi[m]) if a not in avoid and b not in avoid][:count]
    return pairs[0::2], pairs[1::2]


MASK_OFFSETS = (1, 2, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129)


def _join(parts):
    ex = [p for e, _ in parts for p in e]; sp = [p for _, s in parts for p in s]
    return ex, sp


def topology(kind, name, inter="coul", min_visibility=None):
    """(excluded, special) of one family on system `name`; pairs as (lo, hi) tuples.
    masks: offsets MASK_OFFSETS, six pairs each (at least four asserted) — both mask words of both kinds at dl = 0, 1, 63, 64, 127, and ±64/65 over the edge
    far: δ ∈ {200, 500} (those below n) and nothing else: the masks stay empty.   far_wide: the same plus (0, n − 1): xl_span = n − 1
    far_excl: as far, every pair excluded.   mols: long without the hubs.   mols_excl: the two fully excluded molecules and nothing else
    near3: |δ| <= 3 only: xl_span = 3.   far200: δ = 200 only, xl_span = 200: candidates further apart skip the scan
    long: the two fully excluded molecules of the blob system, special pairs from their atoms to outside neighbours (near and far), hubs of 31, 32, 33 entries"""
    ref = bare_reference(name, inter)
    n = ref.n
    pick = lambda d, c=6, **kw: excepted(ref, d, c, min_visibility, **kw)
    if kind in ("masks", "masks_excl", "masks_excl_1sp"):
        parts = [pick(d) for d in MASK_OFFSETS if d < n]
        assert all(len(e) + len(s) >= 4 for e, s in parts), [len(e) + len(s) for e, s in parts]
        ex, sp = _join(parts)
        if kind == "masks_excl": return ex + sp, []                      # no special pair at all: the one-type LJ fluid keeps its byte-offset entries
        if kind == "masks_excl_1sp": return ex + sp[1:], sp[:1]          # one special pair: flagged entries
        return ex, sp
    if kind in ("far", "far_wide", "far_excl"):
        parts = [pick(d, 8) for d in (200, 500) if d < n]
        assert all(len(e) + len(s) >= 2 for e, s in parts)
        ex, sp = _join(parts)
        if kind == "far_excl": return ex + sp, []
        return (ex + [(0, n - 1)], sp) if kind == "far_wide" else (ex, sp)
    if kind == "near3":
        return _join([pick(d, 8) for d in (1, 2, 3)])
    if kind == "far200":
        return _join([pick(200, 12)])
    if kind in ("long", "mols", "mols_excl"):
        blobs = SYSTEMS[name]["blobs"]
        in_blob = np.zeros(n, bool)
        ex, sp = [], []
        for first, m, _ in blobs:
            in_blob[first:first + m] = True
            ex += [(a, b) for a in range(first, first + m) for b in range(a + 1, first + m)]
        if kind == "mols_excl": return ex, []      # the two molecules alone: lists of 39 and 149 excluded entries, no special pair anywhere
        inside = ref.r <= ref.rc
        for first, m, _ in blobs:      # specials from molecule atoms to outside neighbours: behind the molecule's excluded entries in the CSR, at k >= 32
            a_in, b_in = (ref.lo >= first) & (ref.lo < first + m), (ref.hi >= first) & (ref.hi < first + m)
            cross = inside & (a_in ^ b_in) & ~(in_blob[ref.lo] & in_blob[ref.hi])
            d = ref.hi - ref.lo
            near = np.nonzero(cross & (d < 60))[0][:6]; far = np.nonzero(cross & (d > 130))[0][:6]
            assert len(near) >= 3 and len(far) >= 3, (len(near), len(far))
            sp += [(int(ref.lo[k]), int(ref.hi[k])) for k in np.concatenate([near, far])]
        if kind == "mols": return ex, sp          # without the hubs: below 33 partners per atom inside the cutoff there is nobody to make one of
        used = set(np.asarray(sp).reshape(-1).tolist())
        deg = np.bincount(np.concatenate([ref.lo[inside], ref.hi[inside]]), minlength=n)
        hubs = []
        for want in (31, 32, 33):
            for h in np.argsort(-deg, kind="stable"):
                h = int(h)
                nb = np.concatenate([ref.hi[inside & (ref.lo == h)], ref.lo[inside & (ref.hi == h)]])
                nb = [int(b) for b in nb if not in_blob[b] and b not in used]
                if in_blob[h] or h in used or len(nb) < want: continue
                nb = nb[:want]
                ex += [(min(h, b), max(h, b)) for b in nb[0::2]]; sp += [(min(h, b), max(h, b)) for b in nb[1::2]]
                used |= set(nb) | {h}; hubs.append((h, want))
                break
        assert [w for _, w in hubs] == [31, 32, 33]
        return ex, sp
    raise KeyError(kind)


def list_lengths(n, excluded, special):
    """entries per atom of the merged CSR, and the position of every entry in its atom's list (excluded first, then special, each in the order given) —
    how mhip_set_exceptions lays the lists out: {(atom, partner): k}"""
    pos, cnt = {}, np.zeros(n, np.int64)
    for pairs in (excluded, special):
        for i, j in pairs:
            for a, b in ((i, j), (j, i)):
                if (a, b) not in pos:
                    pos[(a, b)] = int(cnt[a]); cnt[a] += 1
    return cnt, pos


def case_with(name, kind, inter="coul", min_visibility=None):
    ex, sp = topology(kind, name, inter, min_visibility) if kind != "none" else ([], [])
    return base_case(name, inter, excluded=np.asarray(ex, dtype=np.int32).reshape(-1, 2), special=np.asarray(sp, dtype=np.int32).reshape(-1, 2))


@functools.lru_cache(maxsize=None)
def reference(name, kind, inter="coul", min_visibility=None, dtype_name="float64"):
    return Reference(case_with(name, kind, inter, min_visibility), np.dtype(dtype_name), geometry=_geometry(name, dtype_name))


def report_visibility(ref, dtype, capped, tag="", chosen=True):
    """The visibility condition of a reference, printed and asserted: half the force of every interacting pair is VISIBLE bars of both its atoms.  capped (the
    systems whose force crosses zero or fades): at most 1 % of the pairs below that, and a wrong verdict on any EXCEPTED pair inside the cutoff — taken as plain,
    as special or as excluded instead of what it is — moves both its atoms by VISIBLE bars; chosen=False (a whole molecule after a run: nobody chose its pairs):
    at most 1 % of the excepted pairs below that"""
    vis = ref.visibility(dtype)
    low = float((vis < VISIBLE).mean())
    print(f"[visibility] {ref.case.name} {np.dtype(dtype).name}{tag}: {len(vis)} interacting pairs, smallest 0.5·|f_ij| / bar {vis.min():.3g}, share below {VISIBLE:g} bars {100 * low:.3f} %")
    if not capped:
        assert vis.min() >= VISIBLE
        return
    assert low <= 0.01
    bar = ref.bar(dtype, jumps=False)
    m = (ref.kind != PLAIN) & (ref.r <= ref.rc)
    ok = 0.5 * ref.wrong_verdict_effect()[m] >= VISIBLE * np.maximum(bar[ref.lo[m]], bar[ref.hi[m]])
    assert m.sum() >= 4 and (np.all(ok) if chosen else ok.mean() >= 0.99)


# every (system, interactions, topology family, least visibility asked of the chosen pairs) that a test uses; the host test checks each against the oracle
CHARGED = ("masks", "far", "far_wide", "near3", "far200")
COMBOS = [("gas1024", "coul", k, None) for k in ("none",) + CHARGED] + \
         [("blobs1024", "coul", k, None) for k in ("none", "masks", "long")] + \
         [("gas2048", "coul", k, None) for k in ("masks", "far")] + \
         [(s, "coul", k, None) for s in ("small540", "tri560") for k in CHARGED + ("long",)] + [("tri2048", "coul", k, None) for k in CHARGED + ("mols",)] + \
         [("lj1024", "lj", k, VISIBLE) for k in ("masks_excl", "masks_excl_1sp", "far_excl", "mols_excl")] + [("gas1024", "rf", k, VISIBLE) for k in ("masks", "far")] + [("blobs1024", "rf", "long", None)]
