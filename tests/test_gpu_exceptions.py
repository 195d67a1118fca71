"""The excluded / special verdicts of the neighbour search (k_build in csrc/kernels.h, set_exceptions in csrc/engine.hip) at their edges, against the plain
numpy reference of tests/exceptions_ref.py (itself checked against the CPU oracle in tests/test_exceptions_host.py).

Why forces: k_export_nl emits a pair from the atom with the lower caller index only, so an exported list shows the verdicts taken with caller-index offset
δ = oj − oi > 0.  The verdicts with δ < 0 — the lower mask words mexc0 / mspc0, half of the full list — are seen by the force kernels alone.  Every system here
is built so that ONE wrong directed entry moves a force by 20 bars or more (exceptions_ref.Reference.visibility, asserted at the top of every case; printed by
the host test), and a failing force check names the atom, its offsets to its excepted partners and the single entry that explains the difference.

Which case runs which line of the search (k_build, `if constexpr (XL)` block and `exception_of`):

  mask bits, dl = δ + 64                    family `masks`: excluded AND special pairs at δ = ±{1, 2, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129}
    dl = 0     (δ = −64, bit 0 of *0)         the pair (i, i + 64) seen from i + 64
    dl = 63    (δ = −1, bit 63 of *0)         the pairs (i, i + 1) seen from i + 1 (`near3` has nothing else there but δ = −2, −3)
    dl = 65    (δ = +1, bit 1 of *1)          the same pairs seen from i; `dl < 64` picks the word, `dl & 63` the bit (dl = 64 is δ = 0, the atom itself: no pair has it)
    dl = 127   (δ = +63, bit 63 of *1)        the pair (i, i + 63) seen from i
    dl = 128   (δ = +64: out of the window)   the pair (i, i + 64) seen from i: `far`, the list scan — a mask bit for one atom, a scan for the other
    dl = −1    (δ = −65)                      (i, i + 65) seen from i + 65: the scan again;  δ = ±66, ±127 … ±129 further out
  far scan                                  families `far`, `far200`, `far_wide` (δ ∈ {200, 500}, n − 1: every mask empty, `far` set), `masks` (|δ| >= 65), `long`
  xl_span skip                              `far200` (span 200: candidates beyond ±200 of an atom with `far` return before the scan), `near3` (span 3, nothing far),
                                            `far_wide` (span n − 1 through the one pair (0, n − 1): nothing skips)
  atoms without exceptions in a wave with atoms that have some       every family but `long`; asserted from mhip_export_order in the `far` cases
  k >= X_cap, mask fold (first `k < A.X_cap ?`)      `long`: special entries of molecule atoms to outside atoms at |δ| < 64, at positions 39+ / 149+ of the list;
                                            the 150-atom molecule's excluded entries 32 … 148 with |δ| < 64; the hub with 33 entries
  k >= X_cap, scan (second `k < A.X_cap ?`) `long`: the same special entries at |δ| > 130, the molecule's excluded entries beyond ±64, hubs (partners anywhere)
  x_part shared by the j-splits             `long`, `masks` and `far` at 64 x 16, 64 x 1 (nothing shared), 128 x 4, 256 x 2 (test_launch_shapes)
  CSR merge in set_exceptions               test_raw_lists_through_the_c_abi: a pair in both lists, three times, in both orders, in the special list before and
                                            after its excluded twin's position; refusals leave the held topology alone
  XL <-> non-XL instantiation, LDS layout   test_live_changes: masks → no exceptions → long → no exceptions on one context
  a molecule with every pair excluded       test_fully_excluded_molecules_feel_nothing_from_inside: against a context whose molecule is switched off instead (ϵ = 0, q = 0)
  `mspc0 &= ~mexc0; mspc1 &= ~mexc1`        no case can reach it: set_exceptions merges a pair's flags into one entry, the fold tests XL_EXCLUDED first (`else if`), and
                                            exception_of reads the excluded word first — the line is a second guard, not a decision

Search paths (what mhip_get_stats can confirm is asserted; the rest is inferred as said):
  dual list <walk, approx, XL> + prune      default: n_filter_passes >= 1 after the first force call, again after 30 steps (n_outer_builds, n_filter_passes grow)
  single exact list <walk, exact, XL>       MOLLYHIP_OUTER_MARGIN_PM=0: n_filter_passes == 0
  in-loop exact minimum image               `small540` (3.4 nm box, r_list 1.2): minimg_mode == 1
  transposed search with XL                 `tri560`: a triclinic cell with heights below 3·r_list has no cell grid, and rebuild_impl takes `walk = false` for it — no
                                            figure in the stats; inferred from that rule (engine.hip: `walk = !no_list && (!tri_mode || tri_grid)`)
  walk on a triclinic cell grid             `tri2048`: heights of 5 nm and more hold 12 cells of r_list / 2; n_blocks > 1 and max_tile_atoms < n say the blocks saw a neighbourhood
  consumers that re-deal entries (fp32)     the group-split pass (reaction field, MOLLYHIP_GROUP_SPLIT=4, n_group_split_passes >= 1: masks, far, long); the one-type LJ fluid with
                                            excluded pairs only at the mask edges, far only, and as two fully excluded molecules (byte-offset entries without a flag bit: engine.hip want_eshift — no figure in the stats, inferred from its rule: fp32, one
                                            atom type, no Coulomb, no special pair) and with one special pair (flagged entries again)

Every family runs on every path; what a path cannot take is said beside its table below.  In short: the hubs of `long` need 31 to 33 partners inside the cutoff, which
tri2048 (0.75 nm: 23) and the LJ fluid (0.6 nm: 12) do not have — they run the molecules without hubs (`mols`, `mols_excl`); δ = 500 exists in every system (the smallest has 540
atoms: 40 index pairs at that offset); fp64 has no group-split pass, no byte-offset entries and at most 512 lanes (64 x 8 for 64 x 16); both consumers are cubic and fp32 only."""
import ctypes as C

import numpy as np
import pytest

from tests import exceptions_ref as X
from tests import systems as S

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


def exported(pkg, s):
    L = pkg.lib()
    n = C.c_int64(0)
    s._check(L.mhip_export_neighbors(s.engine(), None, None, None, 0, C.byref(n)))
    i = np.empty(n.value, np.int32); j = np.empty(n.value, np.int32); sp = np.empty(n.value, np.uint8)
    s._check(L.mhip_export_neighbors(s.engine(), s._ptr(i), s._ptr(j), s._ptr(sp), n.value, C.byref(n)))
    return S.sorted_pairs(i, j, sp)


def assert_same_list(got, ref, tag):
    want = ref.half_list()
    if len(got[0]) == len(want[0]) and all(np.array_equal(u, v) for u, v in zip(got, want)):
        return
    a = set(zip(got[0].tolist(), got[1].tolist(), got[2].tolist())); b = set(zip(want[0].tolist(), want[1].tolist(), want[2].tolist()))
    show = lambda t: [f"({i}, {j}, δ {j - i}, special {sp}, should be {('plain', 'special', 'excluded')[ref.exceptions.get((i, j), 0)]})" for i, j, sp in sorted(t)[:8]]
    raise AssertionError(f"{tag}: exported list differs from the reference: {len(a - b)} entries too many {show(a - b)}, {len(b - a)} missing {show(b - a)}")


def check(pkg, s, ref, dtype, tag, step_n=0, f=None, extra_rel=0.0, energy=True):
    """export, forces, energy and net force of system `s` against the reference"""
    f = np.asarray(pkg.forces(s, step_n=step_n) if f is None else f, dtype=np.float64)
    assert_same_list(exported(pkg, s), ref, tag)
    f_ref = ref.forces()
    df = f - f_ref
    if np.dtype(dtype) == np.float32:
        ratio = np.linalg.norm(df, axis=1) / (ref.bar(np.float32) + extra_rel * np.linalg.norm(f_ref, axis=1))
    else:      # every component within atol 1e-9 + rtol 1e-8·|f_ref|, as numpy's assert_allclose takes it
        ratio = (np.abs(df) / (1e-9 + 1e-8 * np.abs(f_ref))).max(axis=1)
    worst = [int(a) for a in np.argsort(-ratio)[:4] if ratio[a] > 1.0]
    print(f"[exceptions] {tag}: worst per-atom force error / bar {ratio.max():.3g}; net force {np.linalg.norm(f.sum(axis=0)):.3g}, allowed {ref.bar(dtype).sum():.3g}")
    assert not worst, f"{tag}: {int((ratio > 1.0).sum())} atoms over the force bar — " + " | ".join(ref.explain(a, df[a], float(ref.bar(dtype)[a])) for a in worst)
    # Newton's third law: a verdict taken on one side only leaves a net force
    assert np.linalg.norm(f.sum(axis=0)) <= ref.bar(dtype).sum() + extra_rel * np.linalg.norm(f_ref, axis=1).sum()
    if energy:
        e, e_ref = pkg.potential_energy(s, step_n=step_n), ref.potential_energy()
        assert e == pytest.approx(e_ref, rel=1e-10 if np.dtype(dtype) == np.float64 else 2e-5), tag
    return f


def start(pkg, system, kind, dtype, inter="coul", minvis=None):
    ref = X.reference(system, kind, inter, minvis, np.dtype(dtype).name)
    X.report_visibility(ref, dtype, capped=minvis is not None, tag=f" {kind}")
    return ref.case, ref, ref.case.system(pkg, dtype)


def mixed_wave(pkg, s, ref):
    """some 64-atom wave of the sorted order holds atoms with and atoms without exceptions"""
    perm = np.empty(ref.n, np.int32)
    s._check(pkg.lib().mhip_export_order(s.engine(), perm.ctypes.data_as(C.c_void_p), ref.n))
    has = np.zeros(ref.n, bool); has[np.asarray(list(ref.exceptions)).reshape(-1)] = True
    waves = [has[perm[a:a + 64]] for a in range(0, ref.n, 64)]
    return any(w.any() and not w.all() for w in waves)


def set_margin(monkeypatch, single):
    if single: monkeypatch.setenv("MOLLYHIP_OUTER_MARGIN_PM", "0")
    else: monkeypatch.delenv("MOLLYHIP_OUTER_MARGIN_PM", raising=False)


FP = pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
LISTS = pytest.mark.parametrize("single", [False, True], ids=["dual", "single"])
# Every family on the cubic base systems.  `long` needs the two molecules, which blobs1024 has (r_list 1.0 nm, so that a hub finds 33 partners); gas1024 and blobs1024
# are the same kind of box, so masks / far / span kinds are not repeated on blobs1024 here (test_live_changes runs masks on it).
CUBIC = [("gas1024", k) for k in X.CHARGED] + [("blobs1024", "long")]


@FP
@pytest.mark.parametrize("system,kind", CUBIC, ids=[f"{s}-{k}" for s, k in CUBIC])
def test_dual_list(pkg, monkeypatch, system, kind, dtype):
    """<walk, approx, XL>, then the prune: after the first build, and after 30 velocity-Verlet steps of 0.5 fs — prunes and a second outer search carry the flags —
    against the reference on the coordinates the engine holds, which must still show every pair (asserted)"""
    set_margin(monkeypatch, False)
    case, ref, s = start(pkg, system, kind, dtype)
    check(pkg, s, ref, dtype, f"{system} {kind} dual")
    st = s.stats()
    assert st["n_outer_builds"] >= 1 and st["n_filter_passes"] >= 1, st
    if kind.startswith("far"):
        assert mixed_wave(pkg, s, ref)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 30)
    st2 = s.stats()
    print(f"[exceptions] {system} {kind} after 30 steps: searches {st['n_outer_builds']} -> {st2['n_outer_builds']}, prunes {st['n_filter_passes']} -> {st2['n_filter_passes']}")
    assert st2["n_filter_passes"] > st["n_filter_passes"] and st2["n_outer_builds"] > st["n_outer_builds"], (st, st2)
    now = X.Reference(case, dtype, coords=np.asarray(s.coords, dtype=np.float64))
    assert np.abs(now.case.coords - np.asarray(s.coords)).max() > 1e-4       # they moved
    X.report_visibility(now, dtype, capped=False, tag=f" {kind}, after 30 steps")
    assert_same_list(exported(pkg, s), now, f"{system} {kind} dual, the list in use after 30 steps")
    check(pkg, s, now, dtype, f"{system} {kind} dual after 30 steps", step_n=30)


@FP
@pytest.mark.parametrize("system,kind", CUBIC, ids=[f"{s}-{k}" for s, k in CUBIC])
def test_single_exact_list(pkg, monkeypatch, system, kind, dtype):
    """<walk, exact, XL>: one list of radius r_list, the band decisions exact"""
    set_margin(monkeypatch, True)
    case, ref, s = start(pkg, system, kind, dtype)
    check(pkg, s, ref, dtype, f"{system} {kind} single")
    st = s.stats()
    assert st["n_filter_passes"] == 0 and st["n_outer_builds"] >= 1, st


# The other searches take every family too.  tri2048 runs `mols` for `long`: the molecules and their special pairs without the three hubs, because inside its 0.75 nm
# cutoff an atom has 23 partners (29 within r_list) and a hub needs 31 to 33; a longer cutoff would take r_list + the outer margin past what its cell grid is built for.
OTHER = [(s, k) for s in ("small540", "tri560") for k in X.CHARGED + ("long",)] + [("tri2048", k) for k in X.CHARGED + ("mols",)]


@FP
@pytest.mark.parametrize("system,kind", OTHER, ids=[f"{s}-{k}" for s, k in OTHER])
def test_small_box_and_triclinic_searches(pkg, monkeypatch, system, kind, dtype):
    """the in-loop exact minimum image (small540), the transposed search of a triclinic cell without a cell grid (tri560), the walk on a triclinic grid (tri2048)"""
    set_margin(monkeypatch, False)
    case, ref, s = start(pkg, system, kind, dtype)
    check(pkg, s, ref, dtype, f"{system} {kind}")
    st = s.stats()
    print(f"[exceptions] {system}: block_atoms {st['block_atoms']}, j_split {st['j_split']}, blocks {st['n_blocks']}, minimg_mode {st['minimg_mode']}, max_tile_atoms {st['max_tile_atoms']}, prunes {st['n_filter_passes']}")
    if system == "small540":
        assert st["minimg_mode"] == 1, st
    if system == "tri2048":
        assert st["n_blocks"] > 1 and st["max_tile_atoms"] < case.n, st
    if system == "tri560":
        h = 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(case.triclinic["basis"])), axis=0)
        assert h.max() < 3.0 * case.r_list          # fewer than 6 cells of r_list / 2 on every axis: no cell grid


SHAPES = {np.float32: [(64, 16), (64, 1), (128, 4), (256, 2)], np.float64: [(64, 8), (64, 1), (128, 4), (256, 2)]}      # fp64: 512 lanes at the most, so 64 x 8 for 64 x 16
# masks and a far-only family on the 2 048-atom gas (8 blocks of 256), the long lists on blobs1024 (r_list 1.0 nm for the hubs; 4 blocks of 256).  The span kinds
# (far_wide, near3, far200) differ from `far` in one kernel argument, xl_span, which no launch shape touches: they stay with the list tests above.
SHAPE_CASES = [(d, bi, js, s, k) for d in DTYPES for bi, js in SHAPES[d] for s, k in (("gas2048", "masks"), ("gas2048", "far"), ("blobs1024", "long"))]


@pytest.mark.parametrize("dtype,bi,js,system,kind", SHAPE_CASES, ids=[f"{np.dtype(d).name}-{bi}x{js}-{s}-{k}" for d, bi, js, s, k in SHAPE_CASES])
def test_launch_shapes(pkg, monkeypatch, dtype, bi, js, system, kind):
    """the LDS copy of the lists is written by the js == 0 lanes and read by every j-split of the block: shapes with 16, 8, 4, 2 and no j-splits, one to four waves of atoms"""
    set_margin(monkeypatch, False)
    case, ref, s = start(pkg, system, kind, dtype)
    pkg.set_launch_config(s, bi, js)
    check(pkg, s, ref, dtype, f"{system} {kind} {bi} x {js}")
    st = s.stats()
    assert (st["block_atoms"], st["j_split"]) == (bi, js), st


# fp32 only (the engine has byte-offset entries for fp32 alone), cubic only (the one-type kernels know no triclinic cell).  Excluded pairs only keep the entries without
# a flag bit: at the mask edges, far only, and the two fully excluded molecules (lists of 39 and 149 entries; a hub would need 31 partners inside 0.6 nm, an atom has 12).
@pytest.mark.parametrize("kind", ["masks_excl", "masks_excl_1sp", "far_excl", "mols_excl"])
def test_one_type_fluid_with_byte_offset_entries(pkg, monkeypatch, kind):
    """fp32 one-type LJ fluid: with excluded pairs only, the lists hold byte-offset entries without a flag bit; one special pair takes it back to flagged entries.
    The LJ force crosses zero: the excepted pairs are chosen among those a wrong verdict on which shows (asserted), the share of other pairs below 20 bars is capped —
    before the run and after it (of a whole molecule nobody chose the pairs: after the run 99 % of them must show)."""
    set_margin(monkeypatch, False)
    case, ref, s = start(pkg, "lj1024", kind, np.float32, inter="lj", minvis=X.VISIBLE)
    assert int(ref.half_list()[2].sum()) == (1 if kind == "masks_excl_1sp" else 0)
    check(pkg, s, ref, np.float32, f"lj1024 {kind}")
    check(pkg, s, ref, np.float32, f"lj1024 {kind}, second pass (the inner list)")
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 20)
    now = X.Reference(case, np.float32, coords=np.asarray(s.coords, dtype=np.float64))
    X.report_visibility(now, np.float32, capped=True, tag=f" {kind}, after 20 steps", chosen=kind != "mols_excl")
    check(pkg, s, now, np.float32, f"lj1024 {kind} after 20 steps", step_n=20)


# fp32, cubic, dual list only: gs_groups() in engine.hip gives the pass to nothing else.  On blobs1024 with the reaction field every pair shows by 26 bars (the cap is not
# needed), so the long lists run uncapped; the masks and far pairs on gas1024 are chosen among the visible ones as for every capped system.
GS_CASES = [("gas1024", "masks", X.VISIBLE), ("gas1024", "far", X.VISIBLE), ("blobs1024", "long", None)]


@pytest.mark.parametrize("system,kind,minvis", GS_CASES, ids=[f"{s}-{k}" for s, k, _ in GS_CASES])
def test_group_split_pass(pkg, monkeypatch, system, kind, minvis):
    """The group-split pass (forces_gs.hip) re-deals the list entries over four workgroups per block.  It runs only in steps that have bonded terms to fold in, so — as
    tests/test_gpu_pair_physics.py does — the system gets one harmonic bond of strength 0 and atoms so heavy that nothing moves in three velocity-Verlet steps from rest:
    f = m·v / (3 dt) is the force the steps saw (their kicks add 12·2⁻²⁴ relative to the bar).  Reaction field with ϵ_rf = 4 (exceptions_ref.RF_DIELECTRIC).  The
    energy is that of the unmoved system, from the energy call."""
    set_margin(monkeypatch, False)
    monkeypatch.setenv("MOLLYHIP_GROUP_SPLIT", "4")
    mass, dt, steps = float(np.float32(1.0e12)), 0.001, 3
    ref = X.reference(system, kind, "rf", minvis, "float32")
    X.report_visibility(ref, np.float32, capped=minvis is not None, tag=f" {kind}, group split")
    c = ref.case
    heavy = S.Case(c.coords, c.box, lj=c.lj, coul=c.coul, r_list=c.r_list, rebuild_every=c.rebuild_every, velocities=np.zeros((c.n, 3)), charge=c.charge, sigma=c.sigma, eps=c.eps,
                   mass=np.full(c.n, mass), excluded=c.excluded, special=c.special, bonds=dict(i=np.array([0], np.int32), j=np.array([1], np.int32), k=np.zeros(1), r0=np.full(1, 0.3)))
    s = heavy.system(pkg, np.float32)
    x0 = np.array(s.coords, dtype=np.float64)
    pkg.simulate(s, pkg.VelocityVerlet(dt=dt, remove_CM_motion=0), steps)
    st = s.stats()
    assert st["group_split"] == 4 and st["n_group_split_passes"] >= 1, st
    assert np.abs(np.asarray(s.coords, dtype=np.float64) - x0).max() < 1e-9
    f = np.asarray(s.velocities, dtype=np.float64) * (mass / (steps * dt))
    assert_same_list(exported(pkg, s), ref, f"{system} rf {kind}, the list the group-split pass walked")
    check(pkg, s, ref, np.float32, f"{system} rf {kind}, group-split pass", f=f, extra_rel=12 * 2.0 ** -24, step_n=steps)


def raw_call(pkg, s, ex, sp):
    a = lambda p, k: np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1, 2)[:, k])
    exi, exj, spi, spj = a(ex, 0), a(ex, 1), a(sp, 0), a(sp, 1)
    return pkg.lib().mhip_set_exceptions(s.engine(), s._ptr(exi), s._ptr(exj), len(exi), s._ptr(spi), s._ptr(spj), len(spi))


# Families 4 and 5 on the dual and on the single exact list.  set_exceptions builds one CSR on the host before any search, the same buffer for every instantiation and
# launch shape; what differs downstream is covered by the families above, which hand their lists over through this same call.
@LISTS
@FP
def test_raw_lists_through_the_c_abi(pkg, monkeypatch, dtype, single):
    """mhip_set_exceptions itself (the Python layer normalises before the engine sees anything): pairs in both lists (the special twin in front of and behind the
    others of its list), the same pair three times, (j, i) beside (i, j) and alone — excluded wins, one verdict per pair.  An index >= n, a negative one and i == j are refused with
    MHIP_ERR_INVALID, in either list, and the context goes on with the topology it held."""
    set_margin(monkeypatch, single)
    case, ref0, s = start(pkg, "gas1024", "none", dtype)
    n = case.n
    ex0, sp0 = X.topology("masks", "gas1024")
    flip = lambda p: (p[1], p[0])
    at = lambda pairs, d: next(p for p in pairs if p[1] - p[0] == d)
    both = [at(ex0, d) for d in (1, 63, 64, 65, 128)] + [at(sp0, d) for d in (2, 63, 64, 66, 129)]      # in both lists: verdicts from either mask word and from the scan
    thrice = [at(ex0, 31), at(ex0, 127)]; thrice_sp = [at(sp0, 31), at(sp0, 127)]
    ex = ex0 + both[5:] + thrice + [flip(p) for p in thrice] + [flip(at(ex0, 32))]
    sp = both[:3] + sp0 + both[3:5] + [flip(p) for p in both[5:]] + thrice_sp + [flip(p) for p in thrice_sp] + [flip(at(sp0, 33))]
    want = X.Reference(case, dtype, excluded=ex, special=sp, geometry=ref0.geometry)
    assert all(want.exceptions[p] == X.EXCLUDED for p in both + ex0) and all(want.exceptions[p] == X.SPECIAL for p in sp0 if p not in both)
    assert len(want.exceptions) == len(set(ex0 + sp0)) and len(ex) + len(sp) >= len(want.exceptions) + 20
    assert raw_call(pkg, s, ex, sp) == 0
    f_held = check(pkg, s, want, dtype, "raw lists")
    assert (s.stats()["n_filter_passes"] == 0) == single
    for bad in ([(3, n)], [(n, 3)], [(-1, 5)], [(5, -1)], [(7, 7)], ex0[:3] + [(2, n + 5)]):
        for lists in ((bad, []), ([], bad), (ex0[:5], bad)):
            assert raw_call(pkg, s, *lists) == -1, (bad, lists)                  # MHIP_ERR_INVALID
            assert b"exception pair" in pkg.lib().mhip_last_error(s.engine())
    f_after = check(pkg, s, want, dtype, "raw lists, after the refusals")      # (another pass form than the first call's: the same forces to rounding)
    assert np.abs(f_after - f_held).max() <= 1e-4 * np.abs(f_held).max()


@LISTS
@FP
def test_live_changes(pkg, monkeypatch, dtype, single):
    """one context: masks → empty lists → long → empty lists.  The search switches between its instantiations with and without the exception lookups, and the LDS layout changes."""
    set_margin(monkeypatch, single)
    case, ref0, s = start(pkg, "blobs1024", "none", dtype)
    check(pkg, s, ref0, dtype, "live: no exceptions yet")
    for kind in ("masks", "none", "long", "none"):
        ref = X.reference("blobs1024", kind, "coul", None, np.dtype(dtype).name)
        assert raw_call(pkg, s, ref.case.excluded, ref.case.special) == 0
        check(pkg, s, ref, dtype, f"live: {kind}")
    assert (s.stats()["n_filter_passes"] == 0) == single


@FP
def test_fully_excluded_molecules_feel_nothing_from_inside(pkg, monkeypatch, dtype):
    """Family `long`: every internal pair of the 40- and the 150-atom molecule is excluded, so an atom of a molecule feels the outside only.  Witness without any
    exclusion inside the molecule: a second context in which the molecule's OTHER atoms have ϵ = 0 and q = 0 and the molecule's internal pairs are ordinary list
    pairs (the special pairs to the outside and the hubs stay).  The force on the atom must be the same in both — first, middle and last atom of each molecule."""
    set_margin(monkeypatch, False)
    case, ref, s = start(pkg, "blobs1024", "long", dtype)
    f1 = np.asarray(pkg.forces(s), dtype=np.float64)
    f_ref = ref.forces()
    for first, m, _ in X.SYSTEMS["blobs1024"]["blobs"]:
        mol = np.arange(first, first + m)
        inside = lambda p: first <= p[0] < first + m and first <= p[1] < first + m
        ex2 = np.asarray([p for p in case.excluded.tolist() if not inside(p)], dtype=np.int32).reshape(-1, 2)
        assert len(ex2) == len(case.excluded) - m * (m - 1) // 2
        for a in (first, first + m // 2, first + m - 1):
            others = mol[mol != a]
            eps2, q2 = np.array(case.eps), np.array(case.charge)
            eps2[others] = 0.0; q2[others] = 0.0
            twin = S.Case(case.coords, case.box, lj=case.lj, coul=case.coul, r_list=case.r_list, charge=q2, sigma=case.sigma, eps=eps2, mass=case.mass, excluded=ex2, special=case.special)
            ref2 = X.Reference(twin, dtype, geometry=ref.geometry)
            assert np.abs(ref2.forces()[a] - f_ref[a]).max() <= 1e-12 * np.abs(f_ref[a]).max()      # the references agree: nothing from inside
            assert int(((ref2.kind != X.EXCLUDED) & ((ref2.lo == a) | (ref2.hi == a)) & np.isin(ref2.lo, mol) & np.isin(ref2.hi, mol)).sum()) >= 10      # the twin does list its internal partners
            f2 = np.asarray(pkg.forces(twin.system(pkg, dtype)), dtype=np.float64)
            d = np.abs(f2[a] - f1[a])
            if np.dtype(dtype) == np.float32:      # two fp32 evaluations, each within its bar of the same reference value
                assert np.linalg.norm(d) <= ref.bar(dtype)[a] + ref2.bar(dtype)[a], (a, d)
            else:
                assert np.all(d <= 2 * (1e-9 + 1e-8 * np.abs(f_ref[a]))), (a, d)
