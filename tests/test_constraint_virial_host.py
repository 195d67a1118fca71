"""The constraint virial without a GPU: the fp64 restatement of tests/constraint_virial_ref.py against closed forms (a static dimer, a freely
rotating dimer, random rigid waters), its independence of the anchor atom, its λ scaling, and the host side of mhip_constraint_virial — the
prototype in the header, the ctypes signature, the mirror's argument checks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import constraint_virial_ref as V
from tests import constraints_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = np.full(3, 3.0)


def dimer(m1=12.0, m2=1.0, d=0.1, tol=1e-14):
    """two atoms along x, the bond well inside the box (y and z of the bond are exactly zero)"""
    x = np.array([[1.0, 1.2, 0.9], [1.0 + d, 1.2, 0.9]])
    m = np.array([m1, m2])
    d = float(x[1, 0] - x[0, 0])      # the bond as fp64 holds it
    cons = R.Constraints(2, m, BOX, dist=([0], [1], [d]), tol=tol)
    return cons, x, m, d


def test_static_dimer_has_the_closed_form():
    """v = 0: RATTLE takes out the relative acceleration along the bond, Wv = −d μ ((f2/m2 − f1/m1)·r̂) r̂⊗r̂ exactly; the drift is then across the
    bond by θ·d, θ = |a⊥| dt²/d, and SHAKE pulls the bond in by d(√(1 − θ²) − 1): Wp = μ d² (√(1 − θ²) − 1)/dt² r̂⊗r̂ = O(dt²)"""
    cons, x, m, d = dimer()
    f = np.array([[30.0, -20.0, 10.0], [-55.0, 40.0, 25.0]])
    mu = m[0] * m[1] / m.sum()
    rel = f[1] / m[1] - f[0] / m[0]
    rr = np.zeros((3, 3)); rr[0, 0] = 1.0
    wp = {}
    for dt in (0.0005, 0.00025):
        Wv, Wp, A = V.constraint_virial(cons, x, np.zeros((2, 3)), f, m, dt=dt)
        wp[dt] = Wp[0, 0]
        want_v = -d * mu * rel[0] * rr
        assert np.abs(Wv - want_v).max() <= 1e-13 * abs(want_v[0, 0])
        theta = np.hypot(rel[1], rel[2]) * dt * dt / d
        want_p = mu * d * d * (np.sqrt(1.0 - theta * theta) - 1.0) / (dt * dt) * rr
        # SHAKE stops within tol of the length: μ d tol/dt² on Wp
        assert np.abs(Wp - want_p).max() <= 2.0 * mu * d * cons.tol / (dt * dt) + 1e-12 * abs(want_p[0, 0])
        assert A == pytest.approx(abs(Wv[0, 0]) + abs(Wp[0, 0]), rel=1e-12)
    assert wp[0.0005] / wp[0.00025] == pytest.approx(4.0, rel=1e-6) and abs(wp[0.0005]) < 1e-3 * abs(Wv[0, 0])      # O(dt²)


def test_free_rotating_dimer_gives_half_the_centripetal_virial():
    """no force, v ⟂ bond at ω: RATTLE has nothing to do (Wv = 0 exactly), SHAKE pulls the drifted bond in by d(√(1 − (ω dt)²) − 1), so
    Wp = −½ μ ω² d² r̂⊗r̂ · (1 + (ω dt)²/4 + …): HALF of the centripetal −μ ω² d², the reference's definition"""
    cons, x, m, d = dimer()
    mu = m[0] * m[1] / m.sum()
    w = 20.0
    v = np.zeros((2, 3)); v[0, 1] = -w * d * mu / m[0]; v[1, 1] = w * d * mu / m[1]      # about the centre of mass: u = ω d ŷ
    u = v[1, 1] - v[0, 1]
    for dt in (0.0005, 0.00025):
        Wv, Wp, A = V.constraint_virial(cons, x, v, np.zeros((2, 3)), m, dt=dt)
        assert not Wv.any()
        th = u * dt / d
        want = mu * d * d * (np.sqrt(1.0 - th * th) - 1.0) / (dt * dt)
        assert abs(Wp[0, 0] - want) <= 2.0 * mu * d * cons.tol / (dt * dt) + 1e-12 * abs(want)
        ratio = Wp[0, 0] / (-0.5 * mu * u * u)
        assert abs(ratio - (1.0 + th * th / 4.0)) <= th ** 4
        assert np.abs(Wp - np.diag([Wp[0, 0], 0, 0])).max() == 0.0


def rigid_waters(n=300, seed=5, box=BOX):
    """random rigid waters (0.09572 nm arms at 104.52°) as angle clusters (i = H, j = O, k = H), random forces, 300 K velocities"""
    rng = np.random.default_rng(seed)
    t = np.deg2rad(104.52); a = 0.09572
    x = np.zeros((3 * n, 3)); m = np.tile([15.999, 1.008, 1.008], n)
    for w in range(n):
        q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        o = rng.uniform(0, box)
        x[3 * w] = o; x[3 * w + 1] = o + a * q[0]; x[3 * w + 2] = o + a * (np.cos(t) * q[0] + np.sin(t) * q[1])
    x -= box * np.floor(x / box)
    O = 3 * np.arange(n)
    dhh = float(np.sqrt(2 * a * a * (1 - np.cos(t))))
    angle = (O + 1, O, O + 2, np.full(n, a), np.full(n, a), np.full(n, dhh))
    v = rng.normal(size=(3 * n, 3)) * np.sqrt(8.314462618e-3 * 300.0 / m)[:, None]
    f = rng.normal(size=(3 * n, 3)) * 800.0
    return x, v, f, m, angle


def test_random_rigid_waters_symmetric_and_dependent_on_dt():
    x, v, f, m, angle = rigid_waters()
    cons = R.Constraints(len(x), m, BOX, angle=angle, tol=1e-13)
    W = {}
    for dt in (0.0005, 0.00025):
        Wv, Wp, A = V.constraint_virial(cons, x, v, f, m, dt=dt)
        W[dt] = (Wv, Wp)
        # Σ_k loc_k ⊗ m_k Δ_k = Σ_e g_e r_e ⊗ r_e over the cluster's bonds: symmetric but for rounding
        assert np.abs(Wv + Wp - (Wv + Wp).T).max() <= 1e-10 * A
    # the RATTLE part does not know the preview step (the kick and its correction are both ∝ dt); the SHAKE part does, so the step is an argument:
    # 0.9 % of the largest component between 0.0005 and 0.00025 ps here
    assert np.abs(W[0.0005][0] - W[0.00025][0]).max() <= 1e-12 * A
    change = np.abs(W[0.0005][1] - W[0.00025][1]).max() / np.abs(W[0.0005][0] + W[0.0005][1]).max()
    assert 2e-3 < change < 3e-2


def test_anchor_independence_and_lambda_scaling():
    x, v, f, m, angle = rigid_waters(n=40, seed=9)
    cons = R.Constraints(len(x), m, BOX, angle=angle, tol=1e-13)
    Wv, Wp, A = V.constraint_virial(cons, x, v, f, m)
    for anchor in (1, 2):
        Wv2, Wp2, _ = V.constraint_virial(cons, x, v, f, m, anchor=anchor)
        assert max(np.abs(Wv2 - Wv).max(), np.abs(Wp2 - Wp).max()) <= 1e-12 * A
    # one λ on every atom scales the result; a λ < 1 on ONE atom of a cluster scales that whole cluster (the minimum over its atoms)
    lam = np.full(len(x), 0.25)
    Wv3, Wp3, A3 = V.constraint_virial(cons, x, v, f, m, lam=lam)
    assert np.allclose(Wv3, 0.25 * Wv, rtol=1e-13, atol=0) and np.allclose(Wp3, 0.25 * Wp, rtol=1e-13, atol=0) and A3 == pytest.approx(0.25 * A, rel=1e-13)
    lam = np.ones(len(x)); lam[3 * np.arange(0, 40, 2) + 2] = 0.5      # a hydrogen of every other water
    half = R.Constraints(len(x), m, BOX, angle=tuple(np.asarray(c)[0::2] for c in angle), tol=1e-13)
    rest = R.Constraints(len(x), m, BOX, angle=tuple(np.asarray(c)[1::2] for c in angle), tol=1e-13)
    a = V.constraint_virial(half, x, v, f, m); b = V.constraint_virial(rest, x, v, f, m)
    Wv4, Wp4, A4 = V.constraint_virial(cons, x, v, f, m, lam=lam)
    assert np.abs(Wv4 + Wp4 - (0.5 * (a[0] + a[1]) + b[0] + b[1])).max() <= 1e-12 * A


def test_fp32_path_rounds_the_inputs_only():
    x, v, f, m, angle = rigid_waters(n=20, seed=2)
    Wv, Wp, A = V.constraint_virial_as(np.float64, len(x), BOX, x, v, f, m, angle=angle)
    Wv32, Wp32, _ = V.constraint_virial_as(np.float32, len(x), BOX, x, v, f, m, angle=angle)
    dev = np.abs(Wv32 + Wp32 - Wv - Wp).max()
    assert 0 < dev <= 1e-4 * A      # float32 inputs move the result by some 1e-6·A: far above the engine tests' 1e-8·A bar, far below the result


def test_header_declares_the_prototype_and_the_binding_has_it(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mollyhip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+mhip_constraint_virial\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/mollyhip.h does not declare mhip_constraint_virial"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mhip_ctx* ctx", "const void* f_xyz", "int32_t mem_kind", "double dt", "double* virial9", "double* parts18", "int64_t* n_not_converged"]
    import ctypes as C
    res, args = pkg.SIGNATURES["mhip_constraint_virial"]
    assert res is C.c_int32 and len(args) == 7 and args[3] is C.c_double and args[2] is C.c_int32
    assert pkg.lib().mhip_constraint_virial(None, None, 0, 0.0005, None, None, None) == -1      # null context


def test_mirror_validates_its_arguments(pkg):
    s = pkg.System(coords=np.array([[1.0, 1.0, 1.0], [1.1, 1.0, 1.0]]), boundary=pkg.CubicBoundary(3.0), mass=[12.0, 1.0],
                   constraints=(pkg.SHAKE_RATTLE(2, dist_constraints=[pkg.DistanceConstraint(0, 1, 0.1)]),))
    for dt in (0.0, -0.0005, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            pkg.constraint_virial(s, forces=np.zeros((2, 3)), dt=dt)
    for bad in (np.zeros((3, 3)), np.zeros(6), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            pkg.constraint_virial(s, forces=bad)
    # without constraints: zeros, no engine needed
    free = pkg.System(coords=np.zeros((2, 3)) + 1.0, boundary=pkg.CubicBoundary(3.0))
    w, wv, wp = pkg.constraint_virial(free, forces=np.zeros((2, 3)), parts=True)
    assert w.shape == wv.shape == wp.shape == (3, 3) and not w.any() and not wv.any() and not wp.any()
    # the constrained System is still refused by default
    with pytest.raises(pkg.MollyHipError):
        pkg.virial(s)
    with pytest.raises(pkg.MollyHipError):
        pkg.scalar_pressure(s)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_kernel_keeps_its_lane_in_registers_and_uses_no_atomics(tmp_path):
    """k_con_virial<float / double> compiled for gfx950: no scratch memory (a lane carries its cluster's whole trial in double, 18 accumulators on top: an
    executed spill would be the cost to watch, occupancy is not — a block is one wave), and no atomic instruction: the partials are reduced by shuffles and summed
    in a fixed order, so a call repeats its bits"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "constraints.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "molly.jl_amd", "csrc", "constraints.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    table = subprocess.run(["python3", os.path.join(ROOT, "tools", "kernel_resources.py"), str(out), "--filter", "k_con_virial"],
                           check=True, capture_output=True, text=True).stdout
    found = {}
    for line in table.splitlines():
        mt = re.match(r"\s*(\d+)\s+(\d+)\s+\d+\s+(\d+)\s+(\d+)\s+void mhip::.*k_con_virial<(float|double)>", line)
        if mt:
            found[mt.group(5)] = tuple(int(mt.group(k)) for k in (1, 2, 3, 4))
    assert set(found) == {"float", "double"}, table
    for T, (scratch, vgpr, lds, scratch_instr) in found.items():
        assert scratch == 0 and scratch_instr == 0 and lds == 0 and vgpr <= 256, (T, table)
    text = open(out).read()
    bodies = re.findall(r"^(_ZN4mhip\S*k_con_virial\S*):[^\n]*\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert len(bodies) == 2
    for name, body in bodies:
        assert "atomic" not in body, name
        assert re.search(r"^\s+global_store_", body, flags=re.M), name      # (the partials)
