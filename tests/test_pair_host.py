"""tests/pair_ref.py — the plain restatement of one nonbonded pair — validated before it judges a kernel (tests/test_gpu_pair_physics.py): against the C++
oracle on the probe systems (forces, potential energy, virial; every strategy × interaction combination the GPU tests run), against the reference's own
known answers (the numbers of tests/test_oracle_golden.py), and the probe builder's promises: isolated dimers, edge probes clear of the rounding band, every
(distance class, flag) cell filled.  Runs without a GPU."""
import collections
import math

import numpy as np
import pytest

from tests import pair_ref as R
from tests.test_oracle_golden import CUTOFF_ROWS

IDS = [f"{n}-{np.dtype(d).name}" for n, d in R.GPU_CASES]


@pytest.mark.parametrize("name", sorted(R.CASES) + ["grid:" + n for n in sorted(R.GRID_CASES)])
def test_pair_ref_matches_the_oracle(name):
    """pair_ref at fp64 against oracle/oracle.cpp at fp64 on the probe system with fp64 inputs.  Both evaluate the reference's formulas in fp64; each is
    within E64 (pair_ref's own distance from longdouble) of the truth, and the two may order a product differently: the bar of pair_ref.reference_errors with
    k = 4, per atom; the totals of energy and virial against the summed per-dimer bars in the same way."""
    p = R.grid_probe(name[5:], np.float64) if name.startswith("grid:") else R.probe(name, np.float64)
    err = R.reference_errors(p, np.float64)
    ref = R.dimer_reference(p, np.float64)
    hi = err["ref"]
    o = p.case.oracle(np.float64)
    nl = o.neighbors("cell")
    listed = hi["listed"]
    assert len(nl[0]) == int(listed.sum())                                           # one list entry per listed dimer: the dimers are isolated
    f = o.forces(nl)
    tiny = np.finfo(np.float64).tiny
    bar = err["bar_f"](4.0) + tiny
    for atoms, sign in ((p.ib, 1.0), (p.ia, -1.0)):
        d = np.linalg.norm(f[atoms] - sign * ref["f"], axis=1)
        assert np.all(d <= bar), f"{name}: worst {np.max(d / bar):.2f} of the bar"
    zero = R.structural_zero(p)
    assert np.all(f[p.ia][zero] == 0) and np.all(f[p.ib][zero] == 0)
    e = o.potential_energy(nl)
    assert abs(e - float(ref["pe"].sum())) <= float(err["bar_e"](4.0)[listed].sum()) + R.sum_allowance(ref["pe"]) + tiny
    w = o.virial(nl)
    assert np.abs(w - ref["vir"].sum(axis=0)).max() <= float(err["bar_w"](4.0)[listed].sum()) + R.sum_allowance(ref["vir"].reshape(-1, 9)) + tiny


@pytest.mark.parametrize("kind,f_ref,pe_ref", CUTOFF_ROWS)
def test_pair_ref_cutoff_known_answers(kind, f_ref, pe_ref):
    # test/interactions.jl:1587-1630: r = 0.7, rc = 0.8, ra = 0.6, σ = 0.3, ϵ = 0.2; zero past the cutoff (r = 1.0 and 0.95)
    lj = dict(cutoff=R._cut_of(kind, 0.8, 0.6))
    for T, atol in ((np.float64, 1e-9), (np.longdouble, 1e-9), (np.float32, 2e-7)):
        out = R.pair(lj, None, [[0.7, 0, 0], [-1.0, 0, 0], [0.0, 0.95, 0]], *[np.full(3, v) for v in (0, 0, 0.3, 0.3, 0.2, 0.2)], np.zeros(3, bool), T, np.float64)
        f = np.asarray(out["fr"][:, None] * out["dr"], dtype=np.float64)
        assert f[0, 0] == pytest.approx(f_ref, abs=atol) and float(out["pe"][0]) == pytest.approx(pe_ref, abs=atol)
        assert out["fr"].dtype == np.dtype(T) and out["pe"].dtype == np.dtype(T)      # evaluated AT the dtype, not converted to it
        if kind != "none":
            assert np.all(f[1:] == 0) and np.all(np.asarray(out["pe"][1:]) == 0)


def test_pair_ref_interaction_known_answers():
    one = lambda **kw: {k: np.array([v]) for k, v in kw.items()}
    z = np.zeros(1, bool)
    # test/interactions.jl:61-82 (LennardJones), :374-395 (Coulomb)
    a = one(qi=1.0, qj=1.0, si=0.3, sj=0.3, ei=0.2, ej=0.2)
    for r, f_lj, e_lj, f_c, e_c in ((0.3, 16.0, 0.0, 1543.727311, 463.1181933), (0.4, -1.375509739, -0.1170417309, 868.3466125, 347.338645)):
        lj = R.pair(dict(cutoff=("none",)), None, [[r, 0, 0]], special=z, dtype=np.float64, **a)
        assert float(lj["fr"][0]) * r == pytest.approx(f_lj, abs=1e-8) and float(lj["pe"][0]) == pytest.approx(e_lj, abs=1e-9)
        c = R.pair(None, dict(kind="plain", cutoff=("none",)), [[r, 0, 0]], special=z, dtype=np.float64, **a)
        assert float(c["fr"][0]) * r == pytest.approx(f_c, abs=1e-5) and float(c["pe"][0]) == pytest.approx(e_c, abs=1e-5)
    # mixing (test/interactions.jl:15, 18): σ(0.3, 0.2) = 0.25 → V(0.25) = 0; ϵ(0.2, 0.1) = 0.1414… = −V at the minimum; LJZeroShortcut (mixing.jl:7-11)
    m = one(qi=0.0, qj=0.0, si=0.3, sj=0.2, ei=0.2, ej=0.1)
    assert abs(float(R.pair(dict(cutoff=("none",)), None, [[0.25, 0, 0]], special=z, dtype=np.float64, **m)["pe"][0])) < 1e-15
    assert float(R.pair(dict(cutoff=("none",)), None, [[2 ** (1 / 6) * 0.25, 0, 0]], special=z, dtype=np.float64, **m)["pe"][0]) == pytest.approx(-0.14142135623730953, abs=1e-15)
    for kw in (dict(si=0.0, sj=0.3, ei=0.2, ej=0.2), dict(si=0.3, sj=0.3, ei=0.0, ej=0.2)):
        out = R.pair(dict(cutoff=("none",)), None, [[0.3, 0, 0]], special=z, dtype=np.float64, **one(qi=0.0, qj=0.0, **kw))
        assert out["fr"][0] == 0 and out["pe"][0] == 0 and out["S"][0] == 0
    # reaction field (coulomb.jl:748-814) and its special-pair rule; Ewald direct space (coulomb.jl:1384-1441): exact erfc, A&S 7.1.26 within 1.5e-7
    ke, q = R.KE, one(qi=0.4, qj=-0.8, si=0.0, sj=0.0, ei=0.0, ej=0.0)
    r, rc, eps = 0.6, 1.0, 78.3
    krf, crf = (eps - 1) / (2 * eps + 1), 3 * eps / (2 * eps + 1)
    rf = dict(kind="rf", rc=rc, eps_rf=eps, weight_special=0.5)
    out = R.pair(None, rf, [[r, 0, 0]], special=z, dtype=np.float64, **q)
    assert float(out["fr"][0]) == pytest.approx(ke * -0.32 * (1 / r - 2 * krf * r * r) / (r * r), rel=1e-14)
    assert float(out["pe"][0]) == pytest.approx(ke * -0.32 * (1 / r + krf * r * r - crf), rel=1e-14)
    out = R.pair(None, rf, [[r, 0, 0]], special=~z, dtype=np.float64, **q)
    assert float(out["fr"][0]) == pytest.approx(0.5 * ke * -0.32 / r ** 3, rel=1e-14) and float(out["pe"][0]) == pytest.approx(0.5 * ke * -0.32 / r, rel=1e-14)
    out = R.pair(None, dict(kind="rf", rc=rc, eps_rf=math.inf), [[r, 0, 0]], special=z, dtype=np.float64, **q)
    assert float(out["pe"][0]) == pytest.approx(ke * -0.32 * (1 / r + r * r / 2 - 1.5), rel=1e-14)
    alpha = math.sqrt(-math.log(2 * 5e-4))
    assert R.ewald_alpha(1.0, 5e-4, np.float64) == pytest.approx(2.6282608, abs=1e-6)
    for approx, tol in ((True, 2e-7), (False, 1e-14)):
        ew = dict(kind="ewald", rc=1.0, approx=approx, weight_special=R.W14)
        for r in (0.15, 0.4, 0.77, 0.99):
            out = R.pair(None, ew, [[r, 0, 0]], special=z, dtype=np.float64, **q)
            g = math.erfc(alpha * r) + 2 * alpha * r * math.exp(-(alpha * r) ** 2) / math.sqrt(math.pi)
            assert float(out["pe"][0]) / (ke * -0.32 / r) == pytest.approx(math.erfc(alpha * r), abs=tol)
            assert float(out["fr"][0]) / (ke * -0.32 / r ** 3) == pytest.approx(g, abs=2 * tol)
        out = R.pair(None, ew, [[1.0001, 0, 0], [0.3, 0, 0]], special=np.array([False, True]), dtype=np.float64, **{k: np.repeat(v, 2) for k, v in q.items()})
        assert out["fr"][0] == 0 and out["pe"][0] == 0
        assert float(out["fr"][1]) == pytest.approx(R.W14 * ke * -0.32 / 0.3 ** 3, rel=1e-14) and float(out["pe"][1]) == pytest.approx(R.W14 * ke * -0.32 / 0.3, rel=1e-14)


@pytest.mark.parametrize("name,dtype", R.GPU_CASES, ids=IDS)
def test_probe_systems_keep_their_promises(name, dtype):
    """What the GPU tests rely on, for every (case, precision) they run — the builder asserts isolation and the band itself (check_isolated, check_band;
    called again here on the finished system) — plus: the crossing, the size limit, the straddling dimers, the zero set, the jump probes' size."""
    p = R.probe(name, dtype)
    c = p.case
    assert c.n <= 1100 and c.n == 2 * len(p.ia)
    assert np.array_equal(c.coords, c.coords.astype(dtype).astype(np.float64)) and np.array_equal(c.sigma, c.sigma.astype(dtype).astype(np.float64))
    R.check_isolated(p)
    assert R.check_band(p)
    m = ~np.isnan(p.edge)
    assert m.any() and np.all(np.abs(p.r64[m] / p.edge[m] - 1) >= R.BAND[np.dtype(dtype)]) and np.all(np.abs(p.r64[m] / p.edge[m] - 1) < 4 * R.DELTA[np.dtype(dtype)])
    cells = collections.Counter(zip(p.cls.tolist(), p.flag.tolist()))
    if c.n > 16:
        flags = R.CASES[name].get("flags", R.FLAGS)
        assert set(cells) == {(cl, fl) for cl in p.classes for fl in flags} and min(cells.values()) >= 4, cells
    else:
        assert set(cells) == set(R.SMALL_CELLS)
    err = R.reference_errors(p, dtype)
    hi = err["ref"]
    assert p.straddles.sum() >= (1 if c.n <= 16 else 20)                               # some dimers reach across a box face
    fr = np.asarray(hi["fr"], dtype=np.float64)
    zero = R.structural_zero(p)
    assert np.all(fr[zero] == 0) and zero.sum() >= 2
    odd = ~zero & (fr == 0)                                                            # an exact zero nobody drew: only the last δ of a smooth switch, where S(r) underflows
    assert np.all(p.kind[odd] == "edge-") and (not odd.any() or "polynomial" in name or "cubic" in name)
    for cl in p.classes:                                                               # every class as its own system (energy and virial): same promises
        R.probe(name, dtype, only=cl)
    # the probes just inside a jump carry at least 100× the widest force bar of their path (factor 8 packed fp32, 4 one-partner fp32 and fp64)
    j = R.jump_probes(p)
    k = 4 if np.dtype(dtype) == np.float64 else 8
    smooth = name in ("lj_none", "lj_shifted_force", "lj_cubic_spline", "lj_polynomial")       # no jump in the force anywhere: nothing for an inclusion test to lose
    assert j.any() != smooth
    if j.any():
        ratio = np.linalg.norm(np.asarray(hi["f"], dtype=np.float64)[j], axis=1) / err["bar_f"](k)[j]
        assert j.sum() >= 2 and np.all(ratio >= 100), (name, ratio.min())


@pytest.mark.parametrize("name,dtype", R.GRID_GPU_CASES, ids=[f"{n}-{np.dtype(d).name}" for n, d in R.GRID_GPU_CASES])
def test_grid_probe_systems_sit_exactly_on_the_radius(name, dtype):
    """the dimers at exactly a cutoff radius (pair_ref.grid_probe_system): the fp64 distance IS the radius, the same arithmetic in the system's own precision gives
    r² == rc² to the last bit, the reference includes the pair (`<=`), and what is lost by excluding it is at least 100× the widest bar"""
    p = R.grid_probe(name, dtype)
    c = p.case
    T = np.dtype(dtype).type
    assert c.n <= 1100
    dr = R.displacement(c.coords[p.ia], c.coords[p.ib], c.box, dtype, dtype)
    r2 = dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]
    assert r2.dtype == np.dtype(dtype) and np.array_equal(r2, (T(1) * p.radius.astype(T)) ** 2) and np.array_equal(r2.astype(np.float64), p.radius ** 2)
    on = np.char.endswith(p.cls, "=")
    cells = collections.Counter(zip(p.cls[on].tolist(), p.flag[on].tolist()))
    assert min(cells.values()) >= (4 if c.n > 16 else 1) and p.straddles is not None if hasattr(p, "straddles") else True
    err = R.reference_errors(p, dtype)
    assert p.straddles.sum() >= 2
    f = np.linalg.norm(np.asarray(err["ref"]["f"], dtype=np.float64), axis=1)
    zero = R.structural_zero(p)
    assert np.all(f[zero] == 0) and np.all(f[~zero] > 0) and not zero[on & R.jump_probes(p)].any()
    j = R.jump_probes(p) & on
    assert j.sum() >= 2 and np.all(f[j] >= 100 * err["bar_f"](4 if np.dtype(dtype) == np.float64 else 8)[j])
