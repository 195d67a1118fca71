"""The numpy reference of the exception-list tests (tests/exceptions_ref.py) against the project's CPU oracle, and the conditions under which a wrong verdict of
the search kernel must show in the forces — all on the CPU.  For every system and topology that tests/test_gpu_exceptions.py runs:

  * the reference's list (pair set and special flags) equals `oracle.neighbors("brute")`, its forces agree to 1e-10 relative, its energy too;
  * for every interacting pair, half its force is at least 20 bars of both its atoms (fp32: 4e-5·Σ_j|f_ij| + 1e-6, fp64: rtol 1e-8 + atol 1e-9).  The one-type LJ
    fluid and the reaction-field system cannot have that for every pair (the force crosses zero, or fades towards the cutoff): there the EXCEPTED pairs are chosen
    among those that have it, and the share of the other pairs below 20 bars is measured, printed and capped at 1 %;
  * the topologies reach what they are built for: offsets on both sides of every mask edge, lists of 31, 32, 33, 39 and 149+ entries, special entries behind
    position 32 with near and with far offsets, atoms whose every exception is far."""
import numpy as np
import pytest

from tests import exceptions_ref as X
from tests import systems as S

IDS = [f"{s}-{i}-{k}" for s, i, k, _ in X.COMBOS]


@pytest.mark.parametrize("system,inter,kind,minvis", X.COMBOS, ids=IDS)
def test_reference_agrees_with_the_oracle(system, inter, kind, minvis):
    case = X.case_with(system, kind, inter, minvis)
    ref = X.reference(system, kind, inter, minvis)
    o = case.oracle(np.float64)
    nl = o.neighbors("brute")
    a, b = S.sorted_pairs(*nl), ref.half_list()
    assert len(a[0]) == len(b[0]) and all(np.array_equal(u, v) for u, v in zip(a, b))
    f_ref, f = o.forces(nl), ref.forces()
    err = np.abs(f - f_ref).max() / np.abs(f_ref).max()
    e_ref, e = o.potential_energy(nl), ref.potential_energy()
    print(f"[exceptions] {case.name} {kind}: {len(b[0])} pairs, {int(b[2].sum())} special, {len(ref.exceptions)} exceptions; reference against oracle: forces {err:.2e} relative, energy {abs(e - e_ref) / abs(e_ref):.2e}")
    assert err <= 1e-10 and abs(e - e_ref) <= 1e-10 * abs(e_ref)
    # the directed view is the half list seen from both ends
    da, db, dsp, df = ref.directed()
    assert len(da) == 2 * len(b[0]) and np.array_equal(np.bincount(da, minlength=case.n), np.bincount(np.concatenate([b[0], b[1]]), minlength=case.n))
    assert np.allclose(np.bincount(da, weights=df, minlength=case.n), ref.force_scale(), rtol=1e-12)


@pytest.mark.parametrize("system,inter,kind,minvis", X.COMBOS, ids=IDS)
def test_every_list_entry_shows_in_the_forces(system, inter, kind, minvis):
    for dtype in (np.float32, np.float64):
        X.report_visibility(X.reference(system, kind, inter, minvis), dtype, capped=minvis is not None)


def test_base_system_is_the_one_described():
    """1 024 atoms, 4.2 nm, minimum distance 0.27 nm, 23.6 list pairs per atom inside 0.75 nm, pair forces 247 … 2 368 kJ mol⁻¹ nm⁻¹, 171 bars; no pair of a
    static system sits within 2e-6 of its cutoff, where fp32 could take it either way"""
    ref = X.bare_reference("gas1024")
    m = ref.inside()
    assert ref.r.min() >= 0.27 and 23 < 2 * m.sum() / ref.n < 24
    assert 246 < np.abs(ref.f_pair[m]).min() < 248 and 2360 < np.abs(ref.f_pair[m]).max() < 2370
    assert 170 < ref.visibility(np.float32).min() < 172
    d = ref.hi[m] - ref.lo[m]
    assert all(17 <= (d == k).sum() <= 26 for k in (63, 64, 65, 128))
    for name in X.SYSTEMS:
        assert not X.bare_reference(name, "lj" if name.startswith("lj") else "coul").cutoff_jump().any(), name
    # caller order independent of position: neighbours in index are no closer than anybody else
    x = ref.case.coords
    d1 = x[1:] - x[:-1]; d1 -= np.round(d1 / 4.2) * 4.2
    assert np.linalg.norm(d1, axis=1).mean() > 1.5


def test_normalisation_of_raw_lists():
    n = 10
    assert X.normalise(n, [(1, 2)], [(1, 2)]) == {(1, 2): X.EXCLUDED}                                  # in both lists: excluded
    assert X.normalise(n, [(2, 1)], [(2, 1), (1, 2), (3, 4), (4, 3), (3, 4)]) == {(1, 2): X.EXCLUDED, (3, 4): X.SPECIAL}
    assert X.normalise(n, None, np.zeros((0, 2))) == {}
    for bad in ([(3, 3)], [(0, 10)], [(-1, 2)], [(10, 0)]):
        with pytest.raises(ValueError):
            X.normalise(n, bad, None)
        with pytest.raises(ValueError):
            X.normalise(n, None, bad)
    # the oracle takes the same raw forms to the same verdicts
    base = X.base_case("gas1024")
    ref0 = X.bare_reference("gas1024")
    p = [(int(a), int(b)) for a, b in zip(ref0.lo[ref0.inside()][:6], ref0.hi[ref0.inside()][:6])]
    raw_ex = [p[0], p[1], p[1], p[1], (p[2][1], p[2][0]), p[2], p[3]]
    raw_sp = [p[0], (p[3][1], p[3][0]), p[4], (p[4][1], p[4][0]), p[5], p[5]]
    ref = X.Reference(base, excluded=raw_ex, special=raw_sp)
    assert ref.exceptions == {p[0]: X.EXCLUDED, p[1]: X.EXCLUDED, p[2]: X.EXCLUDED, p[3]: X.EXCLUDED, p[4]: X.SPECIAL, p[5]: X.SPECIAL}
    case = S.Case(base.coords, base.box, lj=base.lj, coul=base.coul, r_list=base.r_list, charge=base.charge, sigma=base.sigma, eps=base.eps, mass=base.mass,
                  excluded=np.asarray(raw_ex), special=np.asarray(raw_sp))
    o = case.oracle(np.float64)
    nl = o.neighbors("brute")
    assert all(np.array_equal(u, v) for u, v in zip(S.sorted_pairs(*nl), ref.half_list()))
    assert np.abs(o.forces(nl) - ref.forces()).max() <= 1e-10 * np.abs(ref.forces()).max()


def test_topologies_reach_the_edges_they_are_built_for():
    n = 1024
    ex, sp = X.topology("masks", "gas1024")
    for kind_pairs in (ex, sp):      # every offset in both kinds, so that both the excluded and the special mask words get a bit at each edge, from both ends
        d = {b - a for a, b in kind_pairs}
        assert d == set(X.MASK_OFFSETS), sorted(set(X.MASK_OFFSETS) - d)
    # (i, i + 64): a bit of the upper mask word is out of range for i (dl = 128: the far scan), bit 0 of the lower word for i + 64
    assert any(b - a == 64 for a, b in ex) and any(b - a == 63 for a, b in ex)
    for kind in ("far", "far_wide", "far200"):
        ex, sp = X.topology(kind, "gas1024")
        inside = [(a, b) for a, b in ex + sp if (a, b) != (0, n - 1)]
        assert min(b - a for a, b in inside) >= 200 and len(inside) >= 8          # nothing in the ±64 window: every atom's masks stay empty
        assert max(b - a for a, b in ex + sp) == {"far": 500, "far_wide": n - 1, "far200": 200}[kind]      # xl_span
    ex, sp = X.topology("near3", "gas1024")
    assert max(b - a for a, b in ex + sp) == 3
    # the long lists
    ex, sp = X.topology("long", "blobs1024")
    cnt, pos = X.list_lengths(n, ex, sp)
    ref = X.reference("blobs1024", "long")
    assert np.all(cnt[100:140] >= 39) and np.all(cnt[300:450] >= 149)
    assert sorted(cnt[(cnt >= 31) & (cnt <= 33)].tolist()) == [31, 32, 33]                       # the three hubs, and nobody else near the LDS capacity
    in_mol = lambda a: 100 <= a < 140 or 300 <= a < 450
    behind = [(a, b, k) for (a, b), k in pos.items() if in_mol(a) and not in_mol(b)]          # special entries of molecule atoms: behind their excluded ones
    assert all(k >= 39 for _, _, k in behind)
    assert sum(abs(b - a) < 64 for a, b, _ in behind) >= 6 and sum(abs(b - a) > 64 for a, b, _ in behind) >= 6      # read in the mask loop and in the far scan
    # entries past position 32 whose verdict is taken from the list itself and that a force shows: pairs within the cutoff
    inside = {(int(a), int(b)) for a, b in zip(ref.lo[ref.r <= ref.rc], ref.hi[ref.r <= ref.rc])}
    deep = [(a, b) for (a, b), k in pos.items() if k >= 32 and (min(a, b), max(a, b)) in inside]
    assert sum(abs(b - a) >= 65 for a, b in deep) >= 100 and sum(abs(b - a) < 64 for a, b in deep) >= 100
    # the molecules are compact: most internal pairs of the small one are within r_list; of the large one a third (150 atoms 0.27 nm apart fill a ball of 1.1 nm
    # radius at the least: its far side is beyond any r_list), which is 3 800 excluded pairs that the search meets as candidates
    m = (ref.kind == X.EXCLUDED) & (ref.lo >= 100) & (ref.hi < 140)
    assert m.sum() >= 0.7 * 40 * 39 / 2
    m = (ref.kind == X.EXCLUDED) & (ref.lo >= 300) & (ref.hi < 450)
    print(f"[exceptions] 150-atom molecule: {m.sum()} of {150 * 149 // 2} internal pairs within r_list")
    assert m.sum() >= 0.3 * 150 * 149 / 2
