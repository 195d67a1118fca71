"""mhip_constraint_virial (k_con_virial, csrc/constraints.hip) against the fp64 restatement of tests/constraint_virial_ref.py.

The bar of every comparison, both precisions: max |ΔW_ab| <= 1e-8 · A at dist_tolerance = 1e-13, A = Σ |loc_a · m Δ_b| over every cluster, atom and
component.  At that tolerance the two SHAKE solvers may differ per atom by the tolerance, m·|loc|·tol/dt² ≈ 6e-7 per cluster at dt = 0.0005 against
A ≈ 540 per water (1e-9 · A); fp64 rounding adds some 1e-12 · A.  The engine carries its trial in double on the T inputs it holds, and the restatement
gets exactly those (read back with mhip_get_state and widened), so float32 contexts meet the same bar — 460× below what rounding the inputs to float32
does.  Nothing here is timed."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import constraint_virial_ref as V
from tests import constraints_ref as R

pytestmark = pytest.mark.gpu

DT = V.DEFAULT_DT
TOL = 1e-13
BAR = 1e-8
ERR_INVALID, ERR_STATE = -1, -3
KT300 = 8.314462618e-3 * 300.0


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_case(x, box, m, v=None, dist=None, angle=None, lam=None, tol=TOL, max_iters=25):
    """a Case that never runs a pair pass: a short LJ cutoff keeps the context's lists small, and nothing here asks for forces.
    dist = (i, j, d); angle = (i, j = centre, k, theta, d_ij, d_jk)"""
    from molly_jl_amd.workloads import Case
    n = len(x)
    cons = dict(dist_tolerance=tol, max_iters=max_iters)
    if dist is not None:
        cons["dist"] = dict(i=np.asarray(dist[0], np.int32), j=np.asarray(dist[1], np.int32), d=np.asarray(dist[2], np.float64))
    if angle is not None:
        cons["angle"] = dict(i=np.asarray(angle[0], np.int32), j=np.asarray(angle[1], np.int32), k=np.asarray(angle[2], np.int32),
                             theta=np.asarray(angle[3], np.float64), d_ij=np.asarray(angle[4], np.float64), d_jk=np.asarray(angle[5], np.float64))
    return Case(x, box, lj=dict(cutoff=("distance", 0.3)), r_list=0.35, velocities=np.zeros((n, 3)) if v is None else v, sigma=np.full(n, 0.1), eps=np.zeros(n),
                mass=np.asarray(m, np.float64), lam=lam, constraints=cons if (dist is not None or angle is not None) else None, name="constraint_virial")


def held_state(pkg, s):
    """coordinates and velocities as the context holds them, widened"""
    x = np.zeros((len(s), 3), s.dtype); v = np.zeros((len(s), 3), s.dtype)
    assert pkg.lib().mhip_get_state(s._ctx, ptr(x), ptr(v), 0) == 0
    return x, v


def call(pkg, s, f, dt=DT, device=False):
    """→ (W 3×3 added to zeros, Wv, Wp, n_not_converged) of one mhip_constraint_virial"""
    L = pkg.lib()
    f = np.ascontiguousarray(f, dtype=s.dtype)
    w = np.zeros(9); p18 = np.full(18, np.nan); bad = C.c_int64(-1)
    if device:
        import torch
        fd = torch.tensor(f, device="cuda")
        torch.cuda.synchronize()
        rc = L.mhip_constraint_virial(s._ctx, C.c_void_p(fd.data_ptr()), 1, dt, ptr(w), ptr(p18), C.byref(bad))
    else:
        rc = L.mhip_constraint_virial(s._ctx, ptr(f), 0, dt, ptr(w), ptr(p18), C.byref(bad))
    assert rc == 0, L.mhip_last_error(s._ctx).decode()
    return w.reshape(3, 3), p18[:9].reshape(3, 3), p18[9:].reshape(3, 3), bad.value


def restated(pkg, s, case, f, dt=DT, lam=None):
    """the restatement on what the context holds: its coordinates and velocities, the forces, masses, λ and box in its precision"""
    x, v = held_state(pkg, s)
    c2 = copy.copy(case)
    c2.mass = V.rounded(case.mass, s.dtype); c2.box = V.rounded(case.box, s.dtype)
    cons = R.of_case(c2, tol=TOL)
    cons.max_iters = 100
    return V.constraint_virial(cons, x.astype(np.float64), v.astype(np.float64), V.rounded(f, s.dtype), c2.mass, dt=dt, lam=V.rounded(lam, s.dtype))


def compare(pkg, slack, case, dtype, f, what, dt=DT):
    s = case.system(pkg, dtype)
    s.push_state(velocities=True)
    W, Wv, Wp, bad = call(pkg, s, f, dt)
    rv, rp, A = restated(pkg, s, case, f, dt, case.lam)
    assert bad == 0 and A > 0
    name = f"{what} {np.dtype(dtype).name}"
    slack(f"{name}: W vs restatement", np.abs(W - (rv + rp)).max(), BAR * A)
    slack(f"{name}: Wv vs restatement", np.abs(Wv - rv).max(), BAR * A)
    slack(f"{name}: Wp vs restatement", np.abs(Wp - rp).max(), BAR * A)
    assert np.array_equal(W, Wv + Wp)
    s.close()
    return W, A


def rand_fv(rng, m, f_std=800.0):
    m = np.asarray(m, np.float64)
    return rng.normal(size=(len(m), 3)) * f_std, rng.normal(size=(len(m), 3)) * np.sqrt(KT300 / m)[:, None]


def dimers(n, box, rng, d=0.1):
    """n two-atom clusters at random places and directions; the heavy atom first"""
    o = rng.uniform(0, box, (n, 3)); u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    x = np.empty((2 * n, 3)); x[0::2] = o; x[1::2] = o + d * u
    x -= box * np.floor(x / box)
    m = np.tile([12.011, 1.008], n)
    i = 2 * np.arange(n)
    return x, m, (i, i + 1, np.full(n, d))


def waters(n, box, rng, first=0):
    """n rigid waters as angle clusters (i = H, j = O, k = H), atoms (O, H, H)"""
    t = np.deg2rad(104.52); a = 0.09572
    x = np.zeros((3 * n, 3))
    for w in range(n):
        q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        o = rng.uniform(0, box, 3)
        x[3 * w] = o; x[3 * w + 1] = o + a * q[0]; x[3 * w + 2] = o + a * (np.cos(t) * q[0] + np.sin(t) * q[1])
    x -= box * np.floor(x / box)
    O = first + 3 * np.arange(n)
    return x, np.tile([15.999, 1.008, 1.008], n), (O + 1, O, O + 2, np.full(n, t), np.full(n, a), np.full(n, a))


# ---- 1. every cluster kind -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_cluster_kind_on_the_toy_system(pkg, slack, dtype):
    case = R.toy_system()
    case.constraints = dict(case.constraints, dist_tolerance=TOL)
    f = pkg.forces(case.system(pkg, dtype))
    compare(pkg, slack, case, dtype, f, "toy system, its own forces")


# ---- 2. wave and kind edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind,n", [("dimers", 1), ("dimers", 63), ("dimers", 64), ("dimers", 65), ("waters", 1), ("waters", 64), ("waters", 65)])
def test_wave_edges_of_one_kind(pkg, slack, dtype, kind, n):
    rng = np.random.default_rng(100 + n)
    box = np.full(3, 3.0)
    if kind == "dimers":
        x, m, dist = dimers(n, box, rng); angle = None
    else:
        x, m, angle = waters(n, box, rng); dist = None
    f, v = rand_fv(rng, m)
    compare(pkg, slack, raw_case(x, box, m, v, dist=dist, angle=angle), dtype, f, f"{n} {kind}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_mix_with_two_empty_kinds(pkg, slack, dtype):
    """dimers and angle clusters, no 3- or 4-atom central clusters, and free atoms behind them"""
    rng = np.random.default_rng(7)
    box = np.full(3, 3.0)
    xd, md, dist = dimers(70, box, rng)
    xw, mw, angle = waters(3, box, rng, first=len(xd))
    xf = rng.uniform(0, box, (5, 3))
    x = np.concatenate([xd, xw, xf]); m = np.concatenate([md, mw, np.full(5, 39.9)])
    f, v = rand_fv(rng, m)
    compare(pkg, slack, raw_case(x, box, m, v, dist=dist, angle=angle), dtype, f, "70 dimers + 3 waters + 5 free atoms")


# ---- 3. grid stride -------------------------------------------------------------------------------------------------------------------------
def test_grid_stride_over_66000_dimers(pkg, slack):
    """more than 1 024 blocks × 64 lanes of items: every block strides"""
    rng = np.random.default_rng(3)
    box = np.full(3, 12.0)
    x, m, dist = dimers(66000, box, rng)
    f, v = rand_fv(rng, m)
    compare(pkg, slack, raw_case(x, box, m, v, dist=dist), np.float32, f, "66 000 dimers")


# ---- 4. periodic faces ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_clusters_across_every_periodic_face(pkg, slack, dtype):
    """a water whose oxygen sits just inside each of the six faces with a hydrogen beyond it (wrapped to the far side), and one deep inside"""
    t = np.deg2rad(104.52); a = 0.09572
    box = np.array([2.5, 3.0, 3.5])
    xs = []
    for axis in range(3):
        for side in (0, 1):
            o = box * np.array([0.31, 0.47, 0.59]); o[axis] = 0.02 if side == 0 else box[axis] - 0.02
            e1 = np.zeros(3); e1[axis] = -1.0 if side == 0 else 1.0
            e2 = np.zeros(3); e2[(axis + 1) % 3] = 1.0
            xs += [o, o + a * e1, o + a * (np.cos(t) * e1 + np.sin(t) * e2)]
    o = box * 0.5
    xs += [o, o + a * np.array([1.0, 0, 0]), o + a * np.array([np.cos(t), np.sin(t), 0])]
    x = np.array(xs)
    assert ((x < 0) | (x >= box)).any(axis=1).sum() == 6
    x -= box * np.floor(x / box)
    n = len(x) // 3
    O = 3 * np.arange(n)
    m = np.tile([15.999, 1.008, 1.008], n)
    rng = np.random.default_rng(12)
    f, v = rand_fv(rng, m)
    case = raw_case(x, box, m, v, angle=(O + 1, O, O + 2, np.full(n, t), np.full(n, a), np.full(n, a)))
    compare(pkg, slack, case, dtype, f, "waters across the six faces")      # (a loc taken without the minimum image is a box length long: 25× the result)


# ---- 5. closed forms --------------------------------------------------------------------------------------------------------------------------
# every input exactly representable in float32: the closed forms hold for both precisions as they stand
DIMER_X = np.array([[1.0, 1.25, 0.875], [1.125, 1.25, 0.875]]); DIMER_M = np.array([12.0, 1.0]); DIMER_D = 0.125; DIMER_MU = 12.0 / 13.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_static_dimer_on_the_device(pkg, slack, dtype):
    """Wv = −d μ ((f2/m2 − f1/m1)·r̂) r̂⊗r̂; Wp = μ d² (√(1 − θ²) − 1)/dt² r̂⊗r̂ with θ = |a⊥| dt²/d: O(dt²)"""
    f = np.array([[30.0, -20.0, 10.0], [-55.0, 40.0, 25.0]])
    case = raw_case(DIMER_X, np.full(3, 3.0), DIMER_M, dist=([0], [1], [DIMER_D]))
    s = case.system(pkg, dtype); s.push_state(velocities=True)
    rel = f[1] / DIMER_M[1] - f[0] / DIMER_M[0]
    wp = {}
    for dt in (0.0005, 0.00025):
        W, Wv, Wp, bad = call(pkg, s, f, dt)
        want_v = -DIMER_D * DIMER_MU * rel[0]
        th = np.hypot(rel[1], rel[2]) * dt * dt / DIMER_D
        want_p = DIMER_MU * DIMER_D ** 2 * (np.sqrt(1.0 - th * th) - 1.0) / (dt * dt)
        A = abs(want_v) + abs(want_p)
        slack(f"static dimer dt={dt}: Wv_xx vs closed form", abs(Wv[0, 0] - want_v), BAR * A)
        slack(f"static dimer dt={dt}: Wp_xx vs closed form", abs(Wp[0, 0] - want_p), BAR * A)
        off = np.ones((3, 3), bool); off[0, 0] = False
        assert bad == 0 and not Wv[off].any() and not Wp[off].any()      # loc = (d, 0, 0) exactly
        wp[dt] = Wp[0, 0]
    assert wp[0.0005] / wp[0.00025] == pytest.approx(4.0, rel=1e-6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rotating_dimer_on_the_device(pkg, slack, dtype):
    """no force, u = v2 − v1 = 3.25 ŷ ⟂ bond (ω = 26 ps⁻¹): Wv = 0 exactly, Wp = μ d² (√(1 − (ω dt)²) − 1)/dt² = −½ μ u² (1 + (ω dt)²/4 + …), half
    of the centripetal virial — the reference's definition"""
    v = np.array([[0.0, -0.25, 0.0], [0.0, 3.0, 0.0]])
    case = raw_case(DIMER_X, np.full(3, 3.0), DIMER_M, v, dist=([0], [1], [DIMER_D]))
    s = case.system(pkg, dtype); s.push_state(velocities=True)
    u = 3.25
    for dt in (0.0005, 0.00025):
        W, Wv, Wp, bad = call(pkg, s, np.zeros((2, 3)), dt)
        th = u * dt / DIMER_D
        want = DIMER_MU * DIMER_D ** 2 * (np.sqrt(1.0 - th * th) - 1.0) / (dt * dt)
        assert bad == 0 and not Wv.any()
        slack(f"rotating dimer dt={dt}: Wp_xx vs closed form", abs(Wp[0, 0] - want), BAR * abs(want))
        assert abs(Wp[0, 0] / (-0.5 * DIMER_MU * u * u) - (1.0 + th * th / 4.0)) <= th ** 4 + BAR
        assert np.array_equal(W, Wp) and np.count_nonzero(Wp) == 1


# ---- 6. λ ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lambda_below_one_on_one_atom_scales_its_cluster(pkg, slack, dtype):
    rng = np.random.default_rng(21)
    box = np.full(3, 3.0)
    xd, md, dist = dimers(10, box, rng)
    xw, mw, angle = waters(10, box, rng, first=len(xd))
    x = np.concatenate([xd, xw]); m = np.concatenate([md, mw])
    f, v = rand_fv(rng, m)
    lam = np.ones(len(x)); lam[1] = 0.5; lam[4] = 0.3; lam[20] = 0.25; lam[27] = 0.7; lam[28] = 0.1      # a hydrogen, a heavy atom, an oxygen, both hydrogens of a water
    case = raw_case(x, box, m, v, dist=dist, angle=angle, lam=lam)
    W, A = compare(pkg, slack, case, dtype, f, "λ < 1 in 5 of 20 clusters")
    case1 = raw_case(x, box, m, v, dist=dist, angle=angle)
    W1, A1 = compare(pkg, slack, case1, dtype, f, "the same with λ = 1")
    assert A < A1 and np.abs(W - W1).max() > 1e-3 * A1


# ---- 7. virtual sites -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_four_site_water_with_distributed_forces(pkg, slack, dtype):
    from tests import virtual_sites_ref as VS
    case = VS.tip4p_box(4)
    case.constraints = dict(case.constraints, dist_tolerance=TOL)
    s = case.system(pkg, dtype)
    f = pkg.forces(s)                        # distribute_forces! applied: the sites' rows are zero
    assert not f[3::4].any() and s.virtual_site_info()["three_particle"] == 64
    compare(pkg, slack, case, dtype, f, "64 TIP4P-FB waters")


# ---- 8. read-only -----------------------------------------------------------------------------------------------------------------------------------
def test_the_call_leaves_the_state_and_repeats_its_bits(pkg):
    rng = np.random.default_rng(5)
    case = R.toy_system()
    s = case.system(pkg, np.float32); s.push_state(velocities=True)
    f, _ = rand_fv(rng, case.mass)
    x0, v0 = held_state(pkg, s)
    a = call(pkg, s, f)
    x1, v1 = held_state(pkg, s)
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1)
    b = call(pkg, s, f)
    d = call(pkg, s, f, device=True)
    for k in range(3):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k])
    assert np.abs(a[0]).max() > 0


@pytest.mark.parametrize("langevin", [False, True])
def test_a_chunked_run_continues_across_the_call_bit_for_bit(pkg, langevin):
    """20 steps, the call, 20 steps = 40 steps in two chunks without it; the default tolerance"""
    L = pkg.lib()
    case = R.toy_system()
    f, _ = rand_fv(np.random.default_rng(6), case.mass)

    def run(with_call):
        s = case.system(pkg, np.float32); s.push_state(velocities=True)
        for first in (0, 20):
            rc = L.mhip_langevin_run(s._ctx, first, 20, 0.002, 2.494, 1.0, 1, 11, 1000 + first) if langevin else L.mhip_vv_run(s._ctx, first, 20, 0.002, 1)
            assert rc == 0, L.mhip_last_error(s._ctx).decode()
            if with_call and first == 0:
                assert np.abs(call(pkg, s, f)[0]).max() > 0
        out = held_state(pkg, s)
        assert s.constraint_info()["n_not_converged"] == 0
        return out
    (xa, va), (xb, vb) = run(False), run(True)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)


# ---- 9. refusals and no-ops ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg):
    L = pkg.lib()
    rng = np.random.default_rng(8)
    box = np.full(3, 3.0)
    x, m, angle = waters(2, box, rng)
    f, v = rand_fv(rng, m)
    f = f.astype(np.float64)
    case = raw_case(x, box, m, v, angle=angle)
    s = case.system(pkg, np.float64); s.push_state(velocities=True)
    w = np.zeros(9); p18 = np.zeros(18)
    assert L.mhip_constraint_virial(s._ctx, None, 0, DT, ptr(w), None, None) == ERR_INVALID
    assert L.mhip_constraint_virial(s._ctx, ptr(f), 0, DT, None, None, None) == ERR_INVALID
    for dt in (0.0, -DT, float("inf"), float("nan")):
        assert L.mhip_constraint_virial(s._ctx, ptr(f), 0, dt, ptr(w), None, None) == ERR_INVALID
    assert not w.any()
    assert L.mhip_constraint_virial(s._ctx, ptr(f), 0, DT, ptr(w), None, None) == 0      # the nullable outputs
    once = w.copy()
    assert L.mhip_constraint_virial(s._ctx, ptr(f), 0, DT, ptr(w), ptr(p18), None) == 0  # ADDED to virial9, parts18 written
    assert np.array_equal(w, once + once) and np.array_equal(p18[:9] + p18[9:], once)
    # before set_state; before set_atoms
    s2 = case.system(pkg, np.float64); s2.engine()
    assert L.mhip_constraint_virial(s2._ctx, ptr(f), 0, DT, ptr(w), None, None) == ERR_STATE
    s3 = case.system(pkg, np.float64)
    s3._push_atoms = lambda: None
    s3.engine()
    O = np.array([0, 3], np.int32); d3 = np.array([0.09572, 0.09572, 0.15139] * 2)
    assert L.mhip_set_constraints(s3._ctx, 0, None, None, None, 2, ptr(O + 1), ptr(O), ptr(O + 2), ptr(d3), 1e-8, 1e-8, 25) == 0
    xs, vs = held_state(pkg, s)
    assert L.mhip_set_state(s3._ctx, ptr(xs), ptr(vs), 0) == 0
    assert L.mhip_constraint_virial(s3._ctx, ptr(f), 0, DT, ptr(w), None, None) == ERR_STATE
    # no constraints: success, nothing added, the parts zeroed
    free = raw_case(x, box, m, v).system(pkg, np.float64); free.push_state(velocities=True)
    w[:] = 7.0; p18[:] = 5.0; bad = C.c_int64(3)
    assert L.mhip_constraint_virial(free._ctx, ptr(f), 0, DT, ptr(w), ptr(p18), C.byref(bad)) == 0
    assert (w == 7.0).all() and not p18.any() and bad.value == 0
    assert not pkg.constraint_virial(free, f).any()


def test_solves_stopped_at_max_iters_are_counted_for_the_call_alone(pkg):
    """a rotating water needs more than one M-SHAKE iteration: with max_iters = 1 this call counts it, the step loops' counter does not"""
    rng = np.random.default_rng(9)
    box = np.full(3, 3.0)
    x, m, angle = waters(1, box, rng)
    c = (m[:, None] * x).sum(0) / m.sum()
    v = np.cross(np.array([15.0, -20.0, 10.0]), x - c)
    for max_iters, want in ((1, 1), (25, 0)):
        s = raw_case(x, box, m, v, angle=angle, max_iters=max_iters).system(pkg, np.float64); s.push_state(velocities=True)
        W, Wv, Wp, bad = call(pkg, s, np.zeros((3, 3)))
        assert bad == want and np.abs(Wp).max() > 0
        assert s.constraint_info()["n_not_converged"] == 0


# ---- 10. the protein ----------------------------------------------------------------------------------------------------------------------------------
def test_6mrr_virial_with_the_constraint_term(pkg, slack):
    from molly_jl_amd.workloads import protein_6mrr
    case = protein_6mrr(coulomb="rf", dtype=np.float32, constraints="hbonds", rigid_water=True)
    case.constraints = dict(case.constraints, dist_tolerance=TOL)
    s = case.system(pkg, np.float32)
    with pytest.raises(pkg.MollyHipError):
        pkg.virial(s)
    with pytest.raises(pkg.MollyHipError):
        pkg.pressure(s)
    W = pkg.virial(s, constraints=True)
    # piecewise: the force virial of the same state from a context without constraints, the term from the restatement on the engine's forces
    free = copy.copy(case); free.constraints = None
    sf = free.system(pkg, np.float32)
    Wf = pkg.virial(sf)
    f = pkg.forces(s)
    rv, rp, A = restated(pkg, s, case, f)
    slack("6mrr fp32: virial(constraints=True) vs force virial + restatement", np.abs(W - (Wf + rv + rp)).max(), BAR * A)
    Wc, Wv, Wp = pkg.constraint_virial(s, parts=True)
    slack("6mrr fp32: constraint_virial vs restatement", np.abs(Wc - (rv + rp)).max(), BAR * A)
    assert np.abs(Wc).max() > 0.1 * np.abs(Wf).max()      # as large as the force virial: a pressure without it is wrong
    vol = float(np.prod(case.box))
    vel = s.velocities.astype(np.float64); m = s.masses.astype(np.float64)
    k2 = np.einsum("i,ia,ib->ab", m, vel, vel)
    assert np.allclose(pkg.pressure(s, constraints=True), (k2 + W) / vol, rtol=0, atol=1e-6 * np.abs(W).max() / vol)      # (2K + W)/V with the same W
    assert pkg.scalar_virial(s, constraints=True) == pytest.approx(np.trace(W), rel=1e-6)
    assert pkg.scalar_pressure(s, constraints=True) == pytest.approx(np.trace(k2 + W) / (3 * vol), rel=1e-6)
