"""SHAKE_RATTLE restated in fp64 numpy (the checker of the engine's constrained step loops): the clusters of build_clusters
(constraints.jl:251-344), M-SHAKE and RATTLE per cluster (shake.jl), and velocity Verlet / Langevin with them in the reference's order
(simulators.jl:589-620, 1155-1185).  Forces come from the oracle (OracleSystem.forces), Langevin noise from OracleSystem.randn3.
Clusters of one kind are solved together as a batch: same shape, same constraint pattern."""
import numpy as np

# kind → (atoms, constraint pairs (a, b) in local atom numbers, r = x_b − x_a)
SHAPES = {
    "2": (2, [(0, 1)]),
    "3": (3, [(0, 1), (0, 2)]),
    "4": (4, [(0, 1), (0, 2), (0, 3)]),
    "angle": (3, [(0, 1), (1, 2), (0, 2)]),      # (i, j = centre, k): d_ij, d_jk, d_ik
}


def build_clusters(n_atoms, dist=None, angle=None):
    """dist: (i, j, d) arrays, angle: (i, j, k, d_ij, d_jk, d_ik) arrays, 0-based.  → {kind: (atoms (nc, NA) int, d (nc, NC))}; ValueError
    for what SHAKE_RATTLE refuses (an atom in two clusters, more than three constraints on a centre, a chain, a ring, a linear angle, an index
    out of range)."""
    di, dj, dd = (np.asarray(a) for a in (dist if dist is not None else ([], [], [])))
    parent = list(range(n_atoms))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j, d in zip(di.tolist(), dj.tolist(), dd.tolist()):
        if not (0 <= i < n_atoms and 0 <= j < n_atoms) or i == j or not d > 0:
            raise ValueError("distance constraint out of range, degenerate or of non-positive length")
        parent[find(i)] = find(j)
    comps = {}
    for c, i in enumerate(di.tolist()):
        comps.setdefault(find(i), []).append(c)
    out = {k: ([], []) for k in SHAPES}
    owned = set()
    for edges in comps.values():
        if len(edges) > 3:
            raise ValueError("more than three constraints on one central atom")
        pairs = [(int(di[c]), int(dj[c])) for c in edges]
        centre = pairs[0][0]
        if len(pairs) > 1:
            cands = [a for a in pairs[0] if all(a in p for p in pairs)]
            if not cands:
                raise ValueError("a chain or a ring")
            centre = cands[0]
        others = [p[1] if p[0] == centre else p[0] for p in pairs]
        if len(set(others)) != len(others):
            raise ValueError("the same pair constrained twice")
        kind = str(len(pairs) + 1)
        out[kind][0].append([centre] + others)
        out[kind][1].append([float(dd[c]) for c in edges])
        owned.update([centre] + others)
    if angle is not None:
        for i, j, k, a, b, c in zip(*(np.asarray(x).tolist() for x in angle)):
            if not all(0 <= x < n_atoms for x in (i, j, k)) or len({i, j, k}) < 3:
                raise ValueError("angle constraint out of range or repeating an atom")
            if {i, j, k} & owned:
                raise ValueError("an atom in two clusters")
            if min(a + b - c, b + c - a, a + c - b) <= 1e-6 * (a + b + c):
                raise ValueError("a linear angle")
            owned.update((i, j, k))
            out["angle"][0].append([i, j, k])
            out["angle"][1].append([a, b, c])
    return {k: (np.asarray(a, dtype=np.int64).reshape(-1, SHAPES[k][0]), np.asarray(d, dtype=np.float64).reshape(-1, len(SHAPES[k][1])))
            for k, (a, d) in out.items() if len(a)}


def min_image(d, box):
    return d - box * np.round(d / box)


class Constraints:
    def __init__(self, n_atoms, masses, box, dist=None, angle=None, tol=1e-10, max_iters=100):
        self.box = np.asarray(box, dtype=np.float64)
        self.tol, self.max_iters = tol, max_iters
        self.clusters = build_clusters(n_atoms, dist, angle)
        m = np.asarray(masses, dtype=np.float64)
        self.kinds = []
        for kind, (atoms, d) in self.clusters.items():
            na, pairs = SHAPES[kind]
            a = np.array([p[0] for p in pairs]); b = np.array([p[1] for p in pairs])
            S = np.zeros((na, len(pairs)))            # S[k, e] = [k == b_e] − [k == a_e]
            for e, (pa, pb) in enumerate(pairs):
                S[pb, e] += 1; S[pa, e] -= 1
            im = np.where(m[atoms] > 0, 1.0 / np.where(m[atoms] > 0, m[atoms], 1.0), 0.0)     # (nc, NA)
            K = S[b][None] * im[:, b, None] - S[a][None] * im[:, a, None]                  # (nc, NC, NC)
            self.kinds.append((atoms, d, a, b, S, im, K))
        self.n_constraints = sum(d.shape[0] * d.shape[1] for _, d, *_ in self.kinds)

    def shake(self, x0, x):
        """positions x (drifted from x0) moved along the bonds of x0 until every constraint holds within tol; returns the iterations of the slowest cluster"""
        worst = 0
        for atoms, d, a, b, S, im, K in self.kinds:
            r0 = min_image(x0[atoms[:, b]] - x0[atoms[:, a]], self.box)                    # (nc, NC, 3)
            q = min_image(x[atoms] - x[atoms[:, :1]], self.box)                            # (nc, NA, 3)
            g = np.zeros(d.shape)
            D = np.zeros(q.shape)
            for it in range(self.max_iters + 1):
                p = q + D
                s = p[:, b] - p[:, a]
                s2 = (s * s).sum(-1)
                done = np.abs(np.sqrt(s2) - d) <= self.tol
                act = ~done.all(axis=1)
                if not act.any():
                    break
                worst = max(worst, it + 1)
                J = 2.0 * K * np.einsum("nci,nei->nce", s, r0)
                g[act] += np.linalg.solve(J[act], -(s2 - d * d)[act][..., None])[..., 0]
                D = np.einsum("ke,ne,nk,nei->nki", S, g, im, r0)
            else:
                raise RuntimeError("the reference SHAKE did not converge")
            x[atoms] += D
        return worst

    def rattle(self, x, v):
        """v with no relative velocity along any constrained pair (one linear solve per cluster)"""
        for atoms, d, a, b, S, im, K in self.kinds:
            r = min_image(x[atoms[:, b]] - x[atoms[:, a]], self.box)
            u = v[atoms[:, b]] - v[atoms[:, a]]
            A = K * np.einsum("nci,nei->nce", r, r)
            k = np.linalg.solve(A, -(r * u).sum(-1)[..., None])[..., 0]
            v[atoms] += np.einsum("ke,ne,nk,nei->nki", S, k, im, r)

    def check(self, x, v):
        """(max | |r| − d |, max |v_ij · r_ij| / |r_ij|) over all constraints"""
        e_d = e_v = 0.0
        for atoms, d, a, b, S, im, K in self.kinds:
            r = min_image(x[atoms[:, b]] - x[atoms[:, a]], self.box)
            u = v[atoms[:, b]] - v[atoms[:, a]]
            rn = np.sqrt((r * r).sum(-1))
            e_d = max(e_d, float(np.abs(rn - d).max()))
            e_v = max(e_v, float(np.abs((r * u).sum(-1) / rn).max()))
        return e_d, e_v


def of_case(case, tol=1e-10):
    """the reference's Constraints of a workloads.Case with `constraints` (AngleConstraint's dist_ik by the law of cosines, constraints.jl:47-50)"""
    c = case.constraints
    a, d = c.get("angle"), c.get("dist")
    ang = None
    if a is not None:
        dij = np.asarray(a["d_ij"], dtype=np.float64); djk = np.asarray(a["d_jk"], dtype=np.float64)
        dik = np.array([np.sqrt(p * p + q * q - 2 * p * q * np.cos(t)) for p, q, t in zip(dij.tolist(), djk.tolist(), np.asarray(a["theta"]).tolist())])
        ang = (a["i"], a["j"], a["k"], dij, djk, dik)
    return Constraints(case.n, case.mass, case.box, dist=(d["i"], d["j"], d["d"]) if d is not None else None, angle=ang, tol=tol)


def toy_system(n_side=4, spacing=0.6, seed=3):
    """every cluster kind several times on a lattice (2-, 3- and 4-atom central clusters, rigid triangles), LJ with a 0.9 nm cutoff and
    reaction-field charges; 300 K velocities with the constrained components left in (RATTLE takes them out at the first kick)"""
    from molly_jl_amd.workloads import Case
    rng = np.random.default_rng(seed)
    x, m, q, sig, eps = [], [], [], [], []
    di, dj, dd, ai, aj, ak, th, d1, d2 = [], [], [], [], [], [], [], [], []
    kinds = ["2", "3", "4", "angle"]
    for c, cell in enumerate(np.ndindex(n_side, n_side, n_side)):
        o = (np.asarray(cell) + 0.5) * spacing + rng.uniform(-0.03, 0.03, 3)
        base = len(x)
        kind = kinds[c % 4]
        x.append(o); m.append(12.011 if kind != "angle" else 15.999); q.append(-0.3 if kind != "2" else -0.2); sig.append(0.32); eps.append(0.4)
        n_h = {"2": 1, "3": 2, "4": 3, "angle": 2}[kind]
        dirs = np.linalg.qr(rng.normal(size=(3, 3)))[0].T[:n_h]       # orthogonal arms: no two partners close
        if kind == "angle":      # a water-like triangle: 0.1 nm arms at 104.52°
            u = dirs[0] / np.linalg.norm(dirs[0]); w = dirs[1] - (dirs[1] @ u) * u; w /= np.linalg.norm(w)
            t = np.deg2rad(104.52); dirs = np.array([u, np.cos(t) * u + np.sin(t) * w])
        for h in range(n_h):
            r0 = 0.1 + 0.01 * h
            x.append(o + r0 * dirs[h] / np.linalg.norm(dirs[h])); m.append(1.008); q.append(0.3 / n_h if kind != "2" else 0.2); sig.append(0.1); eps.append(0.05)
            if kind != "angle":
                di.append(base); dj.append(base + 1 + h); dd.append(r0)
        if kind == "angle":
            ai.append(base + 1); aj.append(base); ak.append(base + 2); th.append(np.deg2rad(104.52)); d1.append(0.1); d2.append(0.11)
            x[base + 2] = x[base] + 0.11 * dirs[1]
    x = np.asarray(x); n = len(x); m = np.asarray(m)
    box = np.full(3, n_side * spacing)
    v = rng.normal(size=(n, 3)) * np.sqrt(8.314462618e-3 * 300.0 / m)[:, None]
    cons = dict(dist=dict(i=np.asarray(di, np.int32), j=np.asarray(dj, np.int32), d=np.asarray(dd)),
                angle=dict(i=np.asarray(ai, np.int32), j=np.asarray(aj, np.int32), k=np.asarray(ak, np.int32), theta=np.asarray(th), d_ij=np.asarray(d1), d_jk=np.asarray(d2)))
    excl = np.array([(min(a, b), max(a, b)) for a, b in zip(di, dj)] + [(min(a, b), max(a, b)) for a, b, c in zip(ai, aj, ak) for a, b in ((a, b), (b, c), (a, c))], dtype=np.int32)
    return Case(_wrap(x, box), box, lj=dict(cutoff=("distance", 0.9)), coul=dict(kind="rf", rc=0.9, eps_rf=78.3), r_list=1.1, rebuild_every=10,
                velocities=v, charge=np.asarray(q), sigma=np.asarray(sig), eps=np.asarray(eps), mass=m, excluded=excl, name="constraint_toy", constraints=cons)


def _wrap(x, box):
    return x - box * np.floor(x / box)


def _remove_cm(v, m):
    v -= (m[:, None] * v).sum(0) / m.sum()


def _forces(o, x, general):
    o.coords[:] = x
    nl = o.neighbors() if np.isfinite(o.r_list) and o.r_list > 0 else None
    return o.forces(nl, pairwise=True, specific=True, general=general).astype(np.float64)


def vv_run(o, cons, x, v, n_steps, dt, remove_cm_every=1, first_step=0, general=False):
    """simulate!(sys, VelocityVerlet) with constraints (simulators.jl:547-629), fp64; o: an fp64 OracleSystem of the case (forces only)"""
    box = cons.box; m = o.mass.astype(np.float64)
    x = _wrap(np.array(x, dtype=np.float64), box); v = np.array(v, dtype=np.float64)
    if first_step == 0 and remove_cm_every:
        _remove_cm(v, m)
    a = _forces(o, x, general) / m[:, None]
    for step in range(first_step + 1, first_step + n_steps + 1):
        v += a * (dt / 2)
        cons.rattle(x, v)
        x0 = x.copy()
        x += v * dt
        xu = x.copy()
        cons.shake(x0, x)
        v += (x - xu) / dt
        x = _wrap(x, box)
        a = _forces(o, x, general) / m[:, None]
        v += a * (dt / 2)
        cons.rattle(x, v)
        if remove_cm_every and step % remove_cm_every == 0:
            _remove_cm(v, m)
    return x, v


def langevin_run(o, cons, x, v, n_steps, dt, kT, friction, key, ctr1, remove_cm_every=1, first_step=0, general=False):
    """simulate!(sys, Langevin) with constraints (simulators.jl:1099-1220), fp64, the noise of OracleSystem.randn3 (caller index i → ctr0 = i + 1)"""
    box = cons.box; m = o.mass.astype(np.float64)
    x = _wrap(np.array(x, dtype=np.float64), box); v = np.array(v, dtype=np.float64)
    vs = np.exp(-dt * friction); pref = np.sqrt(1.0 - vs * vs) * np.sqrt(kT)
    ns = np.where(m > 0, pref * np.sqrt(1.0 / np.where(m > 0, m, 1.0)), 0.0)
    if first_step == 0 and remove_cm_every:
        _remove_cm(v, m)
    for step in range(first_step + 1, first_step + n_steps + 1):
        a = _forces(o, x, general) / m[:, None]
        v += a * dt
        cons.rattle(x, v)
        x0 = x.copy()
        x += v * (dt / 2)
        z = np.array([o.randn3(i, key, ctr1) for i in range(len(m))])
        ctr1 += 1
        v = vs * v + z * ns[:, None]
        x += v * (dt / 2)
        xu = x.copy()
        cons.shake(x0, x)
        v += (x - xu) / dt
        x = _wrap(x, box)
        if remove_cm_every and step % remove_cm_every == 0:
            _remove_cm(v, m)
    return x, v
