"""The constraint contribution to the virial restated in fp64 numpy (the checker of mhip_constraint_virial): the reference's trial step of
merge_initial_constraint_virial! (simulators.jl:459-495) on the RATTLE and SHAKE of tests/constraints_ref.py, accumulated per cluster as
accumulate_shake_cluster_virial! does (shake.jl:234-250).

    v  <- RATTLE(x, v)                                   accumulates nothing
    v1 = v + (f/m) dt,  v2 = RATTLE(x, v1)               Wv = (1/dt)  sum_c lambda_c sum_k loc_k (x) m_k (v2_k - v1_k)
    x1 = x + v2 dt,     x2 = SHAKE(x1 | bonds of x)      Wp = (1/dt^2) sum_c lambda_c sum_k loc_k (x) m_k (x2_k - x1_k)

loc_k: the minimum-image vector from the cluster's anchor atom to atom k at the unmoved x; lambda_c: the smallest per-atom lambda of the cluster."""
import numpy as np

from tests import constraints_ref as R

DEFAULT_DT = 0.0005      # default_constraint_preview_dt (simulators.jl:454-457), ps


def constraint_virial(cons, x, v, f, m, dt=DEFAULT_DT, lam=None, anchor=0):
    """cons: constraints_ref.Constraints.  → (Wv, Wp, A): the two parts (3×3, [a, b] = loc_a · impulse_b) and A = Σ over every cluster, atom and
    component of |λ_c loc_a · m Δ_b|, scaled like the parts — the magnitude a rounding or a solver tolerance is measured against.
    anchor: the local number of the atom loc is taken from (0: the reference's; any other changes the result by rounding only, Σ_k impulse_k = 0)."""
    x = np.array(x, dtype=np.float64); v = np.array(v, dtype=np.float64); f = np.asarray(f, dtype=np.float64); m = np.asarray(m, dtype=np.float64)
    cons.rattle(x, v)
    acc = np.where(m[:, None] > 0, f / np.where(m > 0, m, 1.0)[:, None], 0.0)
    v1 = v + acc * dt
    v2 = v1.copy()
    cons.rattle(x, v2)
    x1 = x + v2 * dt
    x2 = x1.copy()
    cons.shake(x, x2)
    Wv = np.zeros((3, 3)); Wp = np.zeros((3, 3)); A = 0.0
    for atoms, *_ in cons.kinds:
        loc = R.min_image(x[atoms] - x[atoms[:, anchor:anchor + 1]], cons.box)                     # (nc, NA, 3)
        lc = np.ones(len(atoms)) if lam is None else np.asarray(lam, dtype=np.float64)[atoms].min(axis=1)
        for W_is_v, delta, scale in ((True, v2 - v1, 1.0 / dt), (False, x2 - x1, 1.0 / (dt * dt))):
            term = scale * np.einsum("n,nka,nkb->nkab", lc, loc, m[atoms][..., None] * delta[atoms])
            if W_is_v:
                Wv += term.sum(axis=(0, 1))
            else:
                Wp += term.sum(axis=(0, 1))
            A += float(np.abs(term).sum())
    return Wv, Wp, A


def rounded(a, dtype):
    """an input as the engine of that precision holds it: rounded to dtype and widened again (None stays None)"""
    return None if a is None else np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def constraint_virial_as(dtype, n_atoms, box, x, v, f, m, dist=None, angle=None, dt=DEFAULT_DT, lam=None, tol=1e-13, max_iters=100, anchor=0):
    """the same fp64 arithmetic on what an engine of precision dtype holds: coordinates, velocities, forces, masses, λ and the box rounded to dtype
    (the constraint lengths are handed over in double and stay).  The engine carries its trial in double on those inputs, so both sides do fp64
    arithmetic on identical numbers."""
    r = lambda a: rounded(a, dtype)
    cons = R.Constraints(n_atoms, r(m), r(box), dist=dist, angle=angle, tol=tol, max_iters=max_iters)
    return constraint_virial(cons, r(x), r(v), r(f), r(m), dt=dt, lam=r(lam), anchor=anchor)
