"""Reciprocal-space PME without the PME: what the oracle's restatement (oracle/pme.h) and the engine (csrc/pme.h) are both judged against, and the systems the
device tests of tests/test_gpu_pme_edges.py are made of.

ewald_reciprocal — the exact reciprocal Ewald sum over wave vectors, from the textbook formula (no mesh, no B-splines, no transform), in numpy float64 or
longdouble.  With m = Σ_d m_d b_d (b_d the reciprocal basis, a_i · b_d = δ_id) and S(m) = Σ_j q_j exp(2πi m · x_j):
    E = ke/(2πV) Σ_{m≠0} exp(−π²m²/α²)/m² |S(m)|²  −  ke α/√π Σ q²  −  ke π (Σq)²/(2Vα²)
    F_i = 2 ke q_i / V · Σ_{m≠0} exp(−π²m²/α²)/m² · m · Im(conj(S(m)) exp(2πi m · x_i))          (the analytic gradient)
    W_ab = −∂E/∂ε_ab under x → (1 + ε)x, basis → basis (1 + ε)ᵀ                                   (4th-order central differences of the energy)
The sum runs over |m_d| ≤ mmax per axis; the terms left out are below exp(−π² (mmax/L)²/α²).

spread_paths — the index arithmetic of the spreading kernel (pme_spread_blocks) per batch of 64 sorted atoms, to tell which of its three paths a batch takes."""
import numpy as np

from tests import systems as S

KE = 138.93545764          # coulomb.jl:16
SUBMESH_CELLS = 6144       # the static LDS sub-mesh of k_pme_spread: 48 KiB of 8-byte fixed-point cells
Q_FIX_MAX = 24.0           # a batch holding |q| beyond this leaves the fixed-point sub-mesh (csrc/pme.h, PmeFix)


def _inv3(b):
    """inverse of a 3×3 matrix in longdouble (numpy.linalg stops at float64)"""
    b = np.asarray(b, dtype=np.longdouble)
    c = np.empty((3, 3), np.longdouble)
    for i in range(3):
        for j in range(3):
            c[j, i] = b[(i + 1) % 3, (j + 1) % 3] * b[(i + 2) % 3, (j + 2) % 3] - b[(i + 1) % 3, (j + 2) % 3] * b[(i + 2) % 3, (j + 1) % 3]
    return c / (b[0] @ c[:, 0])


def _energy_forces(x, q, basis, alpha, ke, mmax, T, want_forces):
    x = np.asarray(x, dtype=T); q = np.asarray(q, dtype=T); basis = np.asarray(basis, dtype=T).reshape(3, 3)
    pi = T(4) * np.arctan(T(1))
    V = abs(basis[0] @ np.cross(basis[1], basis[2]))
    m = np.stack(np.meshgrid(*[np.arange(-mmax, mmax + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    mh = m[np.any(m != 0, axis=1)].astype(T) @ _inv3(basis).astype(T).T          # wave vector of (m_1, m_2, m_3): inv(basis) · m
    m2 = (mh * mh).sum(axis=1)
    A = np.exp(-pi * pi * m2 / (T(alpha) * T(alpha))) / m2
    ph = 2 * pi * (mh @ x.T)                                                       # [wave vector][atom]
    c, s = np.cos(ph), np.sin(ph)
    Sre, Sim = c @ q, s @ q
    e = T(ke) / (2 * pi * V) * (A * (Sre * Sre + Sim * Sim)).sum()
    e += -T(ke) * T(alpha) / np.sqrt(pi) * (q * q).sum() - T(ke) * pi * q.sum() ** 2 / (2 * V * T(alpha) * T(alpha))
    if not want_forces:
        return e, None
    im = Sre[:, None] * s - Sim[:, None] * c                                       # Im(conj(S) e^{iφ_i})
    f = 2 * T(ke) / V * q[:, None] * np.einsum("k,kd,ki->id", A, mh, im)
    return e, f


def ewald_reciprocal(x, q, basis, alpha, ke=KE, mmax=14, dtype=np.float64, h=1e-4):
    """(energy, forces (n, 3), virial (3, 3)) of the reciprocal-space Ewald sum with the self and the net-charge term, as float64 arrays.  basis: rows a_1, a_2, a_3
    (any cell, not only lower-triangular ones)."""
    T = np.dtype(dtype).type
    basis = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    e, f = _energy_forces(x, q, basis, alpha, ke, mmax, T, True)
    w = np.zeros((3, 3))
    x = np.asarray(x, dtype=T); bT = basis.astype(T)
    for a in range(3):
        for b in range(3):
            def at(k):
                g = np.eye(3, dtype=T); g[a, b] += T(k) * T(h)
                return _energy_forces(x @ g.T, q, bT @ g.T, alpha, ke, mmax, T, False)[0]
            w[a, b] = -float((at(-2) - 8 * at(-1) + 8 * at(1) - at(2)) / (12 * T(h)))
    return float(e), np.asarray(f, dtype=np.float64), w


# ---- which path of the spreading kernel a batch takes --------------------------------------------------------------
def place(coords, mesh, box):
    """grid_placement_inner! (ewald.jl:484-493) in the precision of `coords`, as the engine evaluates it for an orthorhombic box: first mesh index per axis and
    the fractional offset behind it"""
    T = coords.dtype.type
    n = np.asarray(mesh, dtype=np.int64)
    inv_l = T(1) / np.asarray(box, dtype=np.float64).astype(T)
    t = coords * inv_l
    t = (t - np.floor(t)) * n.astype(T)
    ti = np.floor(t)
    return ti.astype(np.int64) % n, t - ti


def spread_paths(coords_sorted, q_sorted, mesh, order, box, batch=64, cells=SUBMESH_CELLS):
    """"lds" | "direct" | "empty" per batch of 64 atoms in the engine's sorted order (pme_spread_blocks): the first indices relative to the batch's first atom, folded
    into [−n/2, n/2); the extent of the charged atoms' bounding box plus the order; `fits` (no extent beyond the mesh, at most `cells` cells, no charge beyond the
    fixed-point range).  coords_sorted carries the engine's precision in its dtype."""
    coords_sorted = np.asarray(coords_sorted); assert coords_sorted.dtype in (np.float32, np.float64)
    q = np.asarray(q_sorted, dtype=coords_sorted.dtype)
    n = np.asarray(mesh, dtype=np.int64)
    idx, _ = place(coords_sorted, mesh, box)
    out = []
    for a0 in range(0, len(q), batch):
        i, qq = idx[a0:a0 + batch], q[a0:a0 + batch]
        mine = qq != 0
        if not mine.any():
            out.append("empty"); continue
        h = n >> 1
        rel = i - i[0]
        rel = rel + np.where(rel < -h, n, 0)
        rel = rel - np.where(rel >= n - h, n, 0)
        ext = rel[mine].max(axis=0) - rel[mine].min(axis=0) + order
        q_fix_ok = not np.any(np.abs(qq) > coords_sorted.dtype.type(Q_FIX_MAX))
        fits = q_fix_ok and np.all(ext <= n) and int(ext.prod()) <= cells
        out.append("lds" if fits else "direct")
    return out


# ---- systems --------------------------------------------------------------------------------------------------------
def point_charges(x, q, box, order, mesh, dtype=np.float32, rc=0.9, triclinic=None, name="points"):
    """charges at given places as a Case with Ewald direct space (its α: rc, tolerance 5e-4) and PME of the given order and mesh; coordinates and charges rounded to
    `dtype` so that every precision sees the same inputs"""
    x = np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)
    q = np.asarray(q, dtype=np.float64).astype(dtype).astype(np.float64)
    box = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,)).astype(dtype).astype(np.float64)
    n = len(x)
    return S.Case(x, box, coul=dict(kind="ewald", rc=rc, tol=5e-4), r_list=rc + 0.1, charge=q, mass=np.full(n, 12.0), velocities=np.zeros((n, 3)),
                  pme=dict(order=order, mesh=tuple(int(v) for v in mesh)), triclinic=triclinic, name=name)


def random_charges(n, box, order, mesh, seed=0, net=0.0, dtype=np.float32, basis=None, name=None):
    """n charges of ±0.2 … 1 e at uniformly random places; their sum is `net` (to the rounding of dtype).  basis: a sheared cell (rows), box = its diagonal"""
    rng = np.random.default_rng([seed, n])
    q = rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    q += (net - q.sum()) / n
    s = rng.uniform(0, 1, (n, 3))
    if basis is None:
        return point_charges(s * np.asarray(box), q, box, order, mesh, dtype, name=name or f"random{n}")
    basis = np.asarray(basis, dtype=np.float64).astype(dtype).astype(np.float64)
    return point_charges(s @ basis, q, np.diag(basis), order, mesh, dtype, triclinic=dict(basis=basis, approx_images=False), name=name or f"random{n}_tri")


def oracle_pme(case, dtype=np.float64):
    """(forces, energy, virial) of the oracle's reciprocal space alone"""
    o = case.oracle(dtype)
    return (np.asarray(o.forces(None, pairwise=False, specific=False, general=True, nthreads=8), dtype=np.float64), float(o.potential_energy(None, pairwise=False, general=True)),
            o.virial(None, pairwise=False, specific=False, general=True))


def alpha_of(case, dtype=np.float64):
    return case.inter_dict(dtype)["ewald_alpha"]


def basis_of(case):
    return np.asarray(case.triclinic["basis"], dtype=np.float64) if case.triclinic is not None else np.diag(case.box)


def ratios(f, e, w, f_ref, e_ref, w_ref):
    """(worst ‖Δf_i‖ / largest ‖f_i‖, |ΔE|/|E|, max|ΔW| / max|W|)"""
    return (float(np.linalg.norm(f - f_ref, axis=1).max() / np.linalg.norm(f_ref, axis=1).max()), abs(e - e_ref) / abs(e_ref), float(np.abs(w - w_ref).max() / np.abs(w_ref).max()))
