"""fp64 numpy restatement of what the pair lists' validity checks measure on the device (k_max_disp, the tails of the integrator kernels, the STEP
epilogue of k_forces, k_con_step, the pruning passes' blk_disp2): for stored coordinates X, a snapshot Q and velocities V, all as the engine holds
them (read back in its own precision and widened),
    d² = max_i |minimg(X_i − Q_i)|²        v² = max_i |V_i|² over the owned atoms.
The minimum image is taken per periodic axis in a cubic box and through fractional coordinates with round-to-nearest in a TriclinicBoundary (rows of
`basis` are the cell vectors) — the image of a DISPLACEMENT, which is far below half a cell height, so both are the true nearest image.
Also here: the "runner" bookkeeping of tests/test_gpu_list_checks.py (who holds the maximum, by what factor) and the error bounds of the device
arithmetic, derived from the operations and the number formats alone."""
import numpy as np

EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
F32 = 2.0 ** -23      # the result is cast to float once, whatever the working precision


def minimg(d, box, basis=None):
    """nearest image of the displacement vectors d (n, 3)"""
    d = np.asarray(d, np.float64)
    if basis is None:
        box = np.broadcast_to(np.asarray(box, np.float64), (3,))
        return d - box * np.round(d / box)
    B = np.asarray(basis, np.float64).reshape(3, 3)
    s = d @ np.linalg.inv(B)
    return (s - np.round(s)) @ B


def disp2(X, Q, box, basis=None):
    """per-atom |minimg(X_i − Q_i)|²"""
    e = minimg(np.asarray(X, np.float64) - np.asarray(Q, np.float64), box, basis)
    return (e * e).sum(axis=1)


def speed2(V, n_owned=None):
    V = np.asarray(V, np.float64)[:n_owned]
    return (V * V).sum(axis=1)


def top_two(a):
    """(index of the maximum, the maximum, the next largest entry) of a per-atom array"""
    a = np.asarray(a, np.float64)
    i = int(np.argmax(a))
    rest = np.delete(a, i)
    return i, float(a[i]), float(rest.max()) if len(rest) else 0.0


def tol_d2(dtype, L, d2, triclinic=False):
    """Bound on |device d² − reference d²| for a displacement of square d2 in a box of largest side L, working precision `dtype`, ε = its machine epsilon.
    Both sides start from the same stored numbers.  Device: e = x − q per axis, ONE rounding of a number up to L (an atom that crossed a face: |e| ≈ L):
    ≤ ε/2·L; the image step e − L·rint(e/L) subtracts two numbers within a factor 2 and is exact; so each component carries ≤ ε/2·L, the vector ≤ √3·ε/2·L,
    and d² = |e|² moves by ≤ 2·d·√3·ε/2·L < 2·ε·L·d.  Three products and two sums in T: ≤ 5 roundings of ≤ ε/2 relative, < 3·ε·d²; the cast to float
    2⁻²⁴·d².  Doubled for slack in the constants: 4·ε·L·d + 8·ε·d² + 2⁻²³·d².
    Triclinic: the displacement goes through fractional coordinates, s_k from up to three products and two sums of numbers up to |e|/h ≲ 2 (≤ 4·ε
    absolute each), s − rint(s) exact, then e'_c = Σ_k s_k·B_kc with |B_kc| ≤ L: ≤ 3·4·ε·L = 12·ε·L per component, the vector ≤ √3·12·ε·L, and d² moves by
    ≤ 2·d·√3·12·ε·L < 42·ε·L·d: the first term becomes 48·ε·L·d."""
    eps = EPS[np.dtype(dtype)]
    d = np.sqrt(d2)
    return (48.0 if triclinic else 4.0) * eps * L * d + 8.0 * eps * d2 + F32 * d2


def tol_v2(dtype, v2):
    """three products and two sums in T (≤ 5 roundings of ε/2 relative: < 3·ε·v², rounded up to 4·ε·v²) and one cast to float (2⁻²⁴·v², doubled)"""
    return (4.0 * EPS[np.dtype(dtype)] + F32) * v2


def tol_root(tol_sq, sq):
    """the bound on a square carried to its root: |√a − √b| ≤ |a − b| / √b for a, b > 0 (here / the reference root), generous by the factor 2 of the mean value theorem"""
    return tol_sq / np.sqrt(sq) if sq > 0 else np.sqrt(tol_sq)
