"""The three numbers every pair-list validity decision rests on — the largest |x − x_prune|², |x − x_search|² and |v|², taken on the device — against the
fp64 reference of tests/list_check_ref.py, measuring body by measuring body, and mhip_check_finite, the guard in front of them.

The "runner": one atom at a chosen SORTED slot (mhip_export_order of a throw-away context: the order depends on the coordinates only) gets the velocity
(2, −1, 0.5) nm/ps, or is moved by hand.  It out-moves and out-runs every other atom at least two-fold — asserted in the reference of every case — so a
measuring body that drops it (a partial last wave, a missing second trip of the stride loop, an image not taken, snapshots swapped) is wrong by a factor two
and cannot hide in a tolerance.  The slots sit at the edges of rows (16), waves (64), blocks (B) and of the array (n − 1).

A: the direct call forms mhip_plan_state_dev / mhip_plan_disp2_dev at states handed over with set_state.
B: the measuring launches inside the step loops, read from the MOLLYHIP_DEBUG=1 lines the engine prints for each check and each prune.
C: mhip_check_finite."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import list_check_ref as R
from tests import systems as S
from tests.test_gpu_device_calls import Ctx, _p, HOST

pytestmark = pytest.mark.gpu

DT = 0.002
RUNNER_V = np.array([2.0, -1.0, 0.5])
RUNNER_U = RUNNER_V / np.linalg.norm(RUNNER_V)
ERR_NAN = -7


# ---- the runner ---------------------------------------------------------------------------------------------------------------------------
_ORDERS = {}


def sorted_order(pkg, case, dtype):
    """perm[sorted slot] = caller index, as a context of this case orders its atoms at the first search"""
    key = (case.name, np.dtype(dtype).name, case.coords.tobytes())
    if key not in _ORDERS:
        s = case.system(pkg, dtype)
        pkg.forces(s)
        perm = np.empty(case.n, np.int32)
        s._check(pkg.lib().mhip_export_order(s.engine(), perm.ctypes.data_as(C.c_void_p), case.n))
        s.close()
        assert np.array_equal(np.sort(perm), np.arange(case.n))
        _ORDERS[key] = perm
    return _ORDERS[key]


def to_face(case, atom, dtype, basis=None, gap=0.005):
    """Shift EVERY atom by the same vector so that `atom` comes to lie `gap` nm inside the face the runner flies towards (+x in a cubic box; the sheared +b face of
    a triclinic cell).  A common shift keeps all distances: nothing overlaps."""
    T = np.dtype(dtype).type
    x = case.coords
    if basis is None:
        L = case.box[0]
        x = x + np.array([L - gap - x[atom, 0], 0.0, 0.0])
        x -= np.floor(x / case.box) * case.box
        x = x.astype(T).astype(np.float64)
        x = np.where(x >= case.box, 0.0, x)
    else:
        s = np.linalg.solve(basis.T, x.T).T
        h_b = basis[1, 1]                                    # |b_y|: fractional gap along b that is `gap` nm of perpendicular distance or less
        s = s + np.array([0.0, 1.0 - gap / h_b - s[atom, 1], 0.0])
        s -= np.floor(s)
        x = (s @ basis).astype(T).astype(np.float64)
    case.coords = x
    return case


def give_runner(case, atom, v=RUNNER_V, massless=False):
    case.velocities = case.velocities.copy()
    case.velocities[atom] = v
    if massless:
        case.mass = case.mass.copy(); case.mass[atom] = 0.0
    return case


def assert_runner(per_atom_sq, atom, what):
    """the condition every case rests on, in the reference: the runner holds the maximum and its root is at least twice the next atom's"""
    i, top, nxt = R.top_two(per_atom_sq)
    print(f"[runner] {what}: runner {np.sqrt(per_atom_sq[atom]):.6g}, largest {np.sqrt(top):.6g} (atom {i}), next {np.sqrt(nxt):.6g}")
    assert i == atom and np.sqrt(top) >= 2.0 * np.sqrt(nxt), f"{what}: the runner does not dominate the reference"
    return top


# ---- A: the direct forms ------------------------------------------------------------------------------------------------------------------
def _get(e, n, dtype, vel=True):
    x = np.empty((n, 3), dtype); v = np.empty((n, 3), dtype)
    e.get_state(_p(x), _p(v) if vel else None, HOST)
    return x.astype(np.float64), v.astype(np.float64)


def _moved(x, rng, length, atom, runner_step, dtype, vel=RUNNER_V):
    """everybody 'length' nm in a random direction, the runner runner_step nm along its velocity; rounded to the working precision as set_state will see it"""
    u = rng.normal(size=x.shape); u /= np.linalg.norm(u, axis=1, keepdims=True)
    y = x + length * u
    y[atom] = x[atom] + runner_step * np.asarray(vel) / np.linalg.norm(vel)
    return np.ascontiguousarray(y, dtype=dtype)


def _direct(pkg, case, dtype, atom, basis=None, seed=5, vel=RUNNER_V):
    """The sequence of the module docstring's A.  Returns (triple, pair, reference triple, tolerances, per-atom arrays) — every device number read after ONE
    synchronisation of the caller's stream."""
    n, L = case.n, float(np.max(np.abs(basis))) if basis is not None else float(case.box.max())
    rng = np.random.default_rng(seed)
    st = torch.cuda.Stream()
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            f = np.zeros((n, 3), dtype)
            x0 = np.ascontiguousarray(case.coords, dtype=dtype); v0 = np.ascontiguousarray(case.velocities, dtype=dtype)
            e.set_state(_p(x0), _p(v0), HOST)
            e.forces(0, 0, _p(f), None, HOST)                     # the search and the first prune: both snapshots are X0
            X0, _ = _get(e, n, dtype)
            s0 = e.stats()
            x1 = _moved(X0, rng, 0.002, atom, 0.018, dtype, vel)
            e.set_state(_p(x1), None, HOST)
            e.request_prune()
            e.forces(1, 0, _p(f), None, HOST)                     # prunes again: the inner snapshot becomes X1, the outer stays X0
            X1, _ = _get(e, n, dtype)
            s1 = e.stats()
            x2 = _moved(X1, rng, 0.002, atom, 0.012, dtype, vel)
            v2 = np.ascontiguousarray(give_vel(case.velocities, atom, vel), dtype=dtype)
            e.set_state(_p(x2), _p(v2), HOST)
            X2, V2 = _get(e, n, dtype)
            out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
            out2 = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
            e.plan_state_dev(_p(out3))
            e.plan_disp2_dev(_p(out2))
            got3, got2 = out3.clone(), out2.clone()
        st.synchronize()
        got3, got2 = got3.cpu().numpy().astype(np.float64), got2.cpu().numpy().astype(np.float64)
        s2 = e.stats()
    finally:
        e.close()
    assert (s0["n_outer_builds"], s0["n_filter_passes"]) == (1, 1), s0
    assert (s1["n_outer_builds"], s1["n_filter_passes"]) == (1, 2), s1
    assert (s2["n_outer_builds"], s2["n_filter_passes"]) == (1, 2), s2
    box = case.box
    a_outer, a_inner, a_v = R.disp2(X2, X0, box, basis), R.disp2(X2, X1, box, basis), R.speed2(V2)
    ref = np.array([assert_runner(a_outer, atom, "d(X2, X0)"), assert_runner(a_inner, atom, "d(X2, X1)"), assert_runner(a_v, atom, "|V2|")])
    tol = np.array([R.tol_d2(dtype, L, ref[0], basis is not None), R.tol_d2(dtype, L, ref[1], basis is not None), R.tol_v2(dtype, ref[2])])
    return got3, got2, ref, tol


def give_vel(v, atom, vel=RUNNER_V):
    v = np.array(v, np.float64)
    v[atom] = vel
    return v


def _check_direct(slack, got3, got2, ref, tol, tag):
    """Tolerance (list_check_ref.tol_d2 / tol_v2, derived there from the operations): 4·ε·L·d + 8·ε·d² + 2⁻²³·d² for the two displacements (48·ε·L·d in a
    sheared cell), (4·ε + 2⁻²³)·v² for the speed.  The three targets are 0.03² , 0.012² and 5.25: a swap of the snapshots is a factor 6."""
    print(f"[direct {tag}] plan_state_dev {got3}, plan_disp2_dev {got2}, reference {ref}, tolerance {tol}")
    names = ("max |x - x_search|^2", "max |x - x_prune|^2", "max |v|^2")
    for k in range(3):
        slack(f"{tag}: plan_state_dev {names[k]} vs fp64 reference", abs(got3[k] - ref[k]), tol[k])
    for k in range(2):
        slack(f"{tag}: plan_disp2_dev {names[k]} vs fp64 reference", abs(got2[k] - ref[k]), tol[k])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("slot", ["0", "15", "16", "63", "64", "255", "256", "n-1"])
def test_direct_forms_at_every_edge_slot(pkg, slack, slot, dtype):
    """729 atoms: a partial last wave and a partial last block of either call form (1024- and 256-lane blocks); the runner at each row, wave and block edge"""
    case = S.lj_fluid(9, dtype=dtype)
    s = case.n - 1 if slot == "n-1" else int(slot)
    atom = int(sorted_order(pkg, case, dtype)[s])
    _check_direct(slack, *_direct(pkg, case, dtype, atom), f"lj729 slot {slot} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_direct_forms_runner_wrapped_between_snapshot_and_check(pkg, slack, dtype):
    """the runner starts 0.005 nm inside the +x face and crosses it with its first move: both displacements are the 0.03 and 0.012 nm it flew, not L minus that"""
    case = S.lj_fluid(9, dtype=dtype)
    atom = int(np.argmax(case.coords[:, 0]))
    to_face(case, atom, dtype)
    assert case.box[0] - case.coords[atom, 0] < 0.01
    got3, got2, ref, tol = _direct(pkg, case, dtype, atom)
    assert abs(np.sqrt(ref[0]) - 0.03) < 1e-3 and abs(np.sqrt(ref[1]) - 0.012) < 1e-3
    _check_direct(slack, got3, got2, ref, tol, f"lj729 wrapped {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_direct_forms_on_a_sheared_face(pkg, slack, dtype):
    """TriclinicBoundary with the cell grid and the dual list (4096 atoms of the suite's sheared fluid): the runner leaves through the sheared +b face, where
    the image is a lattice vector with x and y components"""
    from tests.test_gpu_triclinic import sheared_fluid
    basis, case = sheared_fluid(dtype, n_side=16)
    s = np.linalg.solve(basis.T, case.coords.T).T
    atom = int(np.argmax(s[:, 1]))
    to_face(case, atom, dtype, basis=basis)
    vel = np.array([2.0, 1.0, 0.5])      # (the runner's velocity mirrored in y: it flies towards +b)
    assert np.linalg.solve(basis.T, vel)[1] > 0
    got3, got2, ref, tol = _direct(pkg, case, dtype, atom, basis=basis, vel=vel)
    assert abs(np.sqrt(ref[0]) - 0.03) < 1e-3 and abs(np.sqrt(ref[1]) - 0.012) < 1e-3
    _check_direct(slack, got3, got2, ref, tol, f"sheared cell {np.dtype(dtype).name}")


def test_direct_forms_second_trip_of_the_stride_loop(pkg, slack):
    """531 441 atoms, fp32: more than 512·1024 lanes (plan_state_dev) and more than 1024·256 (plan_disp2_dev); the runner in the last sorted slot is reached only
    by a second trip of either grid-stride loop.  One force pass and no run; the snapshots are both X0 (no second prune: the two displacements coincide, the
    swap is covered by the small cases)."""
    dtype = np.float32
    case = S.lj_fluid(81, dtype=dtype)
    n = case.n
    assert n > 512 * 1024 and n > 1024 * 256
    atom = int(sorted_order(pkg, case, dtype)[n - 1])
    st = torch.cuda.Stream()
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            f = np.zeros((n, 3), dtype)
            x0 = np.ascontiguousarray(case.coords, dtype=dtype); v0 = np.ascontiguousarray(case.velocities, dtype=dtype)
            e.set_state(_p(x0), _p(v0), HOST)
            e.forces(0, 0, _p(f), None, HOST)
            X0, _ = _get(e, n, dtype)
            x2 = X0.copy(); x2[atom] += 0.03 * RUNNER_U
            x2 = np.ascontiguousarray(x2, dtype=dtype)
            v2 = np.ascontiguousarray(give_vel(case.velocities, atom), dtype=dtype)
            e.set_state(_p(x2), _p(v2), HOST)
            X2, V2 = _get(e, n, dtype)
            out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
            out2 = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
            e.plan_state_dev(_p(out3)); e.plan_disp2_dev(_p(out2))
            got3, got2 = out3.clone(), out2.clone()
        st.synchronize()
        got3, got2 = got3.cpu().numpy().astype(np.float64), got2.cpu().numpy().astype(np.float64)
        s2 = e.stats()
    finally:
        e.close()
    assert (s2["n_outer_builds"], s2["n_filter_passes"]) == (1, 1), s2
    a_d, a_v = R.disp2(X2, X0, case.box), R.speed2(V2)
    assert np.count_nonzero(a_d) == 1      # (nobody else moved at all)
    d2, v2r = assert_runner(a_d, atom, "d(X2, X0)"), assert_runner(a_v, atom, "|V2|")
    L = float(case.box.max())
    ref = np.array([d2, d2, v2r]); tol = np.array([R.tol_d2(dtype, L, d2), R.tol_d2(dtype, L, d2), R.tol_v2(dtype, v2r)])
    _check_direct(slack, got3, got2, ref, tol, "lj531441 slot n-1 float32")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_direct_forms_without_the_dual_list_report_infinity(pkg, monkeypatch, dtype):
    """a context without the dual list (no outer margin) has no plan to vouch for: +inf, +inf — "re-plan at every rebuild step" — and the speed all the same"""
    monkeypatch.setenv("MOLLYHIP_OUTER_MARGIN_PM", "0")
    case = S.lj_fluid(9, dtype=dtype)
    n = case.n
    st = torch.cuda.Stream()
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            f = np.zeros((n, 3), dtype)
            x0 = np.ascontiguousarray(case.coords, dtype=dtype); v0 = np.ascontiguousarray(case.velocities, dtype=dtype)
            e.set_state(_p(x0), _p(v0), HOST)
            e.forces(0, 0, _p(f), None, HOST)
            out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
            out2 = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
            e.plan_state_dev(_p(out3)); e.plan_disp2_dev(_p(out2))
            got3, got2 = out3.clone(), out2.clone()
        st.synchronize()
        got3, got2 = got3.cpu().numpy(), got2.cpu().numpy()
        assert e.stats()["n_filter_passes"] == 0
    finally:
        e.close()
    assert np.isposinf(got3[0]) and np.isposinf(got3[1]) and np.isposinf(got2).all(), (got3, got2)
    assert got3[2] == 0.0      # (documented: the triple is zeroed, then the first two words set to +inf; no kernel runs)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_direct_forms_without_lists_and_past_the_margin(pkg, dtype):
    """No set_state voids the lists by itself: the engine looks at what moved at its next force pass (lists_after_set_state).  So the voided state of the
    direct calls is a context that holds no searched list — a fresh one: +inf, +inf.  And an atom handed over 0.15 nm away, beyond half the 0.2 nm outer
    margin, is REPORTED as a value by a call in front of that pass (the snapshots still stand: that number is what tells the host to re-plan); the pass
    then searches again, and the displacements are 0."""
    case = S.lj_fluid(9, dtype=dtype)
    n = case.n
    atom = int(sorted_order(pkg, case, dtype)[n - 1])
    st = torch.cuda.Stream()
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            f = np.zeros((n, 3), dtype)
            x0 = np.ascontiguousarray(case.coords, dtype=dtype); v0 = np.ascontiguousarray(case.velocities, dtype=dtype)
            e.set_state(_p(x0), _p(v0), HOST)
            out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
            out2 = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
            e.plan_state_dev(_p(out3)); e.plan_disp2_dev(_p(out2)); fresh3, fresh2 = out3.clone(), out2.clone()
            e.forces(0, 0, _p(f), None, HOST)
            X0, _ = _get(e, n, dtype)
            x1 = X0.copy(); x1[atom] += 0.15 * RUNNER_U
            x1 = np.ascontiguousarray(x1, dtype=dtype)
            e.set_state(_p(x1), None, HOST)
            X1, _ = _get(e, n, dtype)
            e.plan_state_dev(_p(out3)); before = out3.clone()
            e.forces(1, 0, _p(f), None, HOST)
            e.plan_state_dev(_p(out3)); after = out3.clone()
        st.synchronize()
        fresh3, fresh2 = fresh3.cpu().numpy(), fresh2.cpu().numpy()
        before, after = before.cpu().numpy().astype(np.float64), after.cpu().numpy().astype(np.float64)
        s1 = e.stats()
    finally:
        e.close()
    print(f"[voided] fresh {fresh3} {fresh2}, before the pass {before}, after {after}, stats outer {s1['n_outer_builds']} prunes {s1['n_filter_passes']}")
    assert np.isposinf(fresh3[:2]).all() and np.isposinf(fresh2).all(), (fresh3, fresh2)
    d2 = R.disp2(X1, X0, case.box)[atom]
    L = float(case.box.max())
    assert np.all(np.abs(before[:2] - d2) <= R.tol_d2(dtype, L, d2)), (before, d2)
    assert s1["n_outer_builds"] == 2, s1      # 0.15 nm > half the 0.2 nm margin: the pass searched again
    assert after[0] == 0.0 and after[1] == 0.0, after


# ---- B: the measuring launches of the step loops -------------------------------------------------------------------------------------------
MEASURED = re.compile(r"\[mhip\] step (\d+): measured at (\d+): d ([0-9.eE+-]+) d_outer ([0-9.eE+-]+) v_max ([0-9.eE+-]+)")
LAZY = re.compile(r"\[mhip\] step (\d+): max disp ([0-9.eE+-]+) nm since the build of step (\d+) \(skin [0-9.]+\), v_max ([0-9.eE+-]+)")
PRUNE = re.compile(r"\[mhip\] prune(?: \(read late\))?: max disp ([0-9.eE+-]+) nm")
HALF_D, HALF_V = 0.5e-5, 0.5e-4      # half a unit of the last printed digit: %.5f nm, %.4f nm/ps


def _debug_run(pkg, case, dtype, sim, n_steps, capfd, monkeypatch, rng=None, launch=None):
    """the run under MOLLYHIP_DEBUG=1 (read once, when the context is made): stderr of the engine and what the run did"""
    monkeypatch.setenv("MOLLYHIP_DEBUG", "1")
    s = case.system(pkg, dtype)
    try:
        s.engine()
        if launch is not None:
            pkg.set_launch_config(s, *launch)
        capfd.readouterr()
        pkg.simulate(s, sim, n_steps, rng=rng)
        err = capfd.readouterr().err
        info = dict(stats=s.stats(), thermostat=s.thermostat_info(), constraints=s.constraint_info() if s.constraints else None)
    finally:
        s.close()
        monkeypatch.delenv("MOLLYHIP_DEBUG")
    print(err)
    return err, info


def _quiet_states(pkg, case, dtype, sim, steps, rng=None, launch=None):
    """the same case in a quiet context, stopped after each of `steps` (ascending): {0: wrapped start, k: (x_k, v_k)} in the engine's precision, widened, and
    the stats at each stop.  VV runs are continued in chunks (a run cut into chunks repeats the uncut run bit for bit: tests/test_gpu_cadence.py,
    test_gpu_device_calls.py); a run that draws noise starts afresh from the same seed for every stop."""
    out, stats = {}, {}
    s = case.system(pkg, dtype)
    try:
        s.engine()
        if launch is not None:
            pkg.set_launch_config(s, *launch)
        s.push_state(); s.pull_state()
        out[0] = (s.coords.astype(np.float64), s.velocities.astype(np.float64))
        if rng is None:
            done = 0
            for k in steps:
                pkg.simulate(s, sim, k - done, init_step=done)
                done = k
                out[k] = (s.coords.astype(np.float64), s.velocities.astype(np.float64)); stats[k] = s.stats()
    finally:
        s.close()
    if rng is not None:
        for k in steps:
            s = case.system(pkg, dtype)
            try:
                s.engine()
                if launch is not None:
                    pkg.set_launch_config(s, *launch)
                pkg.simulate(s, sim, k, rng=rng)
                out[k] = (s.coords.astype(np.float64), s.velocities.astype(np.float64)); stats[k] = s.stats()
            finally:
                s.close()
    return out, stats


def _check_measured(slack, pkg, case, dtype, sim, capfd, monkeypatch, atom, tag, *, rng=None, launch=None, S_at=None, half_step_v=True, cm_term=0.0, proves=None, dt=DT, wrapped=False):
    """One run of S + 2 steps under MOLLYHIP_DEBUG=1; the line "step S+1: measured at S" against the state a quiet context reaches after S steps.

    What the launch measures (integrate.h, kernels.h, constraints.hip): the coordinates x_S it has just made, against both snapshots, and the velocity it
    holds at that moment.  In the velocity-Verlet forms that is the half-step velocity v_{S−1/2} (the first kick of step S is done, the closing one is not),
    which the reference takes from two stored states as minimg(x_S − x_{S−1}) / dt; in the Langevin forms the update is complete and it is v_S.
    Snapshots: both are the wrapped initial coordinates as long as no prune or search ran before the measuring launch — the stats of the quiet run stopped
    at S − 1, whose last launch is the measuring one's twin, must show one search and one prune.
    Tolerance: half a unit of the last printed digit (%.5f nm, %.4f nm/ps) plus the arithmetic bound of A carried to the root (tol / reference root), plus —
    half-step velocity only — the reference's own error: x_S = fl(x_{S−1} + fl(v·dt)) and the wrap each round to an ulp of a coordinate up to L, so
    the difference quotient carries ≤ 2·ε·L / dt per axis, √3 times that on the norm.  cm_term: |v_cm|·dt for positions measured while a removal is pending."""
    every = case.rebuild_every
    S_at = every if S_at is None else S_at
    err, info = _debug_run(pkg, case, dtype, sim, S_at + 2, capfd, monkeypatch, rng=rng, launch=launch)
    if proves is not None:
        proves(info)
    lines = [m for m in MEASURED.finditer(err) if int(m.group(2)) == S_at]
    assert len(lines) == 1 and int(lines[0].group(1)) in (S_at + 1, S_at + 2), err      # (read one or two steps behind the launch that measured)
    d, d_outer, v_max = (float(lines[0].group(k)) for k in (3, 4, 5))
    states, stats = _quiet_states(pkg, case, dtype, sim, (S_at - 1, S_at), rng=rng, launch=launch)
    st = stats[S_at - 1]
    assert (st["n_outer_builds"], st["n_filter_passes"]) == (1, 1), st      # nothing but the search and the prune of step 0 before the measuring launch
    basis = None if case.triclinic is None else np.asarray(case.triclinic["basis"], np.float64)
    L = float(np.max(np.abs(basis))) if basis is not None else float(case.box.max())
    X0, XS, VS = states[0][0], states[S_at][0], states[S_at][1]
    a_d = R.disp2(XS, X0, case.box, basis)
    if half_step_v:
        a_v = (R.minimg(XS - states[S_at - 1][0], case.box, basis) ** 2).sum(axis=1) / dt ** 2
        v_ref_err = np.sqrt(3.0) * 2.0 * R.EPS[np.dtype(dtype)] * L / dt
    else:
        a_v, v_ref_err = R.speed2(VS), 0.0
    if wrapped:      # the runner really crossed the face (+x; the sheared +b face of a triclinic cell) between the snapshot and the check
        f0, fS = (X0[atom, 0] / case.box[0], XS[atom, 0] / case.box[0]) if basis is None else (np.linalg.solve(basis.T, X0[atom])[1], np.linalg.solve(basis.T, XS[atom])[1])
        assert f0 > 0.99 and fS < 0.05, (X0[atom], XS[atom])
    d2 = assert_runner(a_d, atom, f"{tag}: d(x_{S_at}, x_0)")
    v2 = assert_runner(a_v, atom, f"{tag}: speed at the measuring launch")
    tol_d = HALF_D + R.tol_root(R.tol_d2(dtype, L, d2, basis is not None), d2) + cm_term
    tol_v = HALF_V + R.tol_root(R.tol_v2(dtype, v2), v2) + v_ref_err
    print(f"[measured {tag}] printed d {d} d_outer {d_outer} v_max {v_max}; reference {np.sqrt(d2):.9g} {np.sqrt(v2):.9g}; tolerances {tol_d:.3g} {tol_v:.3g}")
    slack(f"{tag}: printed d vs reference, nm", abs(d - np.sqrt(d2)), tol_d)
    slack(f"{tag}: printed d_outer vs reference, nm", abs(d_outer - np.sqrt(d2)), tol_d)
    slack(f"{tag}: printed v_max vs reference, nm/ps", abs(v_max - np.sqrt(v2)), tol_v)
    return info


def _runner_fluid(pkg, n_side, dtype, slot, wrap=False, rebuild_every=10, massless=False):
    case = S.lj_fluid(n_side, dtype=dtype, rebuild_every=rebuild_every)
    if wrap:
        atom = int(np.argmax(case.coords[:, 0]))
        to_face(case, atom, dtype)
    else:
        s = case.n - 1 if slot == "n-1" else int(slot)
        atom = int(sorted_order(pkg, case, dtype)[s])
    return give_runner(case, atom, massless=massless), atom


# The packed pass that integrates wants block-local coordinates: a block's half extent + 1.25·(r_list + margin) below L / 2 on every axis (k_build), which 64-atom
# blocks of this fluid meet at 21³ = 9261 atoms (L = 7.6 nm) and 128-atom blocks do not; those run at the 41³ = 68 921 atoms of the stride-loop cases.  A partial last
# block either way.
STEP_SIDE = {64: 21, 128: 41}
VV0 = lambda pkg: pkg.VelocityVerlet(dt=DT, remove_CM_motion=0)


@pytest.mark.parametrize("slot", ["0", "15", "16", "63", "64", "255", "256", "n-1", "wrap"])
def test_vv_mid_fp64(pkg, slack, capfd, monkeypatch, slot):
    """k_vv_mid (256-lane blocks), the fp64 fluid of 729 atoms: no pair pass integrates in fp64 (n_fused_steps == 0), the stand-alone launch measures"""
    case, atom = _runner_fluid(pkg, 9, np.float64, slot, wrap=slot == "wrap")
    def proves(info): assert info["stats"]["n_fused_steps"] == 0, info["stats"]
    _check_measured(slack, pkg, case, np.float64, VV0(pkg), capfd, monkeypatch, atom, f"k_vv_mid fp64 slot {slot}", proves=proves, wrapped=slot == "wrap")


@pytest.mark.parametrize("slot", ["0", "15", "16", "63", "64", "255", "256", "n-1", "wrap"])
def test_vv_mid_fp32_unfused(pkg, slack, capfd, monkeypatch, slot):
    """k_vv_mid in fp32: MOLLYHIP_FUSE_STEP=0 keeps the pair pass from integrating (n_fused_steps == 0)"""
    monkeypatch.setenv("MOLLYHIP_FUSE_STEP", "0")
    case, atom = _runner_fluid(pkg, 9, np.float32, slot, wrap=slot == "wrap")
    def proves(info): assert info["stats"]["n_fused_steps"] == 0, info["stats"]
    _check_measured(slack, pkg, case, np.float32, VV0(pkg), capfd, monkeypatch, atom, f"k_vv_mid fp32 slot {slot}", proves=proves, wrapped=slot == "wrap")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_vv_mid_second_trip_of_the_stride_loop(pkg, slack, capfd, monkeypatch, dtype):
    """68 921 atoms: the stage kernels' grid is capped at 256 blocks of 256 lanes, so sorted slots >= 65 536 are reached by a second trip; runner at n − 1"""
    monkeypatch.setenv("MOLLYHIP_FUSE_STEP", "0")
    case, atom = _runner_fluid(pkg, 41, dtype, "n-1")
    assert case.n - 1 >= 65536
    def proves(info): assert info["stats"]["n_fused_steps"] == 0, info["stats"]
    _check_measured(slack, pkg, case, dtype, VV0(pkg), capfd, monkeypatch, atom, f"k_vv_mid {np.dtype(dtype).name} 68921 atoms slot n-1", proves=proves)


@pytest.mark.parametrize("block_atoms", [64, 128])
@pytest.mark.parametrize("slot", ["0", "15", "16", "63", "64", "B-1", "B", "n-1", "wrap"])
def test_forces_step_epilogue(pkg, slack, capfd, monkeypatch, slot, block_atoms):
    """the STEP epilogue of k_forces (fp32 one-type fluid, defaults): n_fused_steps > 0 and the block size as set; rows of 16 lanes, waves of 64, blocks of B"""
    sl = {"B-1": str(block_atoms - 1), "B": str(block_atoms)}.get(slot, slot)
    case, atom = _runner_fluid(pkg, STEP_SIDE[block_atoms], np.float32, sl, wrap=slot == "wrap")
    def proves(info):
        assert info["stats"]["n_fused_steps"] >= case.rebuild_every and info["stats"]["block_atoms"] == block_atoms, info["stats"]
    _check_measured(slack, pkg, case, np.float32, VV0(pkg), capfd, monkeypatch, atom, f"k_forces STEP B {block_atoms} slot {slot}", launch=(block_atoms, 4), proves=proves, wrapped=slot == "wrap")


def test_forces_step_epilogue_68921_atoms(pkg, slack, capfd, monkeypatch):
    """the same at the size where the stage kernels would take a second trip: the epilogue has one lane per atom, the last block is partial"""
    case, atom = _runner_fluid(pkg, 41, np.float32, "n-1")
    def proves(info): assert info["stats"]["n_fused_steps"] >= case.rebuild_every, info["stats"]
    _check_measured(slack, pkg, case, np.float32, VV0(pkg), capfd, monkeypatch, atom, "k_forces STEP 68921 atoms slot n-1", proves=proves)


@pytest.mark.parametrize("slot", ["0", "15", "16", "63", "64", "n-1", "wrap"])
def test_forces_step_epilogue_langevin(pkg, slack, capfd, monkeypatch, slot):
    """the LANG form of the epilogue under mhip_langevin_run: the update is complete when it measures, the speed is v_S of the stored state"""
    case, atom = _runner_fluid(pkg, STEP_SIDE[64], np.float32, slot, wrap=slot == "wrap")
    sim = pkg.Langevin(dt=DT, temperature=85.0, friction=1.0, remove_CM_motion=0)
    def proves(info): assert info["stats"]["n_fused_steps"] >= case.rebuild_every, info["stats"]
    _check_measured(slack, pkg, case, np.float32, sim, capfd, monkeypatch, atom, f"k_forces STEP LANG slot {slot}", rng=31, half_step_v=False, proves=proves, wrapped=slot == "wrap")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("slot", ["0", "255", "256", "n-1", "wrap"])
def test_vv_open_behind_a_thermostat(pkg, slack, capfd, monkeypatch, slot, dtype):
    """ImmediateThermostat on every step: the integrator stage is a close and an open launch, and k_vv_open measures (thermostat_info: applied on every step)"""
    monkeypatch.setenv("MOLLYHIP_FUSE_STEP", "0")
    case, atom = _runner_fluid(pkg, 9, dtype, slot, wrap=slot == "wrap")
    sim = pkg.VelocityVerlet(dt=DT, remove_CM_motion=0, coupling=pkg.ImmediateThermostat(temperature=85.0))
    n_run = case.rebuild_every + 2
    def proves(info): assert info["thermostat"]["n_applied"] == n_run and info["stats"]["n_fused_steps"] == 0, info
    _check_measured(slack, pkg, case, dtype, sim, capfd, monkeypatch, atom, f"k_vv_open {np.dtype(dtype).name} slot {slot}", proves=proves, wrapped=slot == "wrap")


def test_vv_mid_while_a_cm_removal_is_pending(pkg, slack, capfd, monkeypatch):
    """remove_CM_motion=1: the launch that measures x_S has the removal of step S − 1 applied, that of step S is still pending — the positions it measures
    are the step's to within |v_cm|·dt, v_cm = Σ m v / Σ m of the reference state (tiny after the removal of step 0)"""
    dtype = np.float64
    case, atom = _runner_fluid(pkg, 9, dtype, "n-1")
    sim = pkg.VelocityVerlet(dt=DT, remove_CM_motion=1)
    states, _ = _quiet_states(pkg, case, dtype, sim, (case.rebuild_every,))
    v = states[case.rebuild_every][1]
    v_cm = np.linalg.norm((case.mass[:, None] * v).sum(axis=0) / case.mass.sum())
    def proves(info): assert info["stats"]["n_fused_steps"] == 0, info["stats"]
    _check_measured(slack, pkg, case, dtype, sim, capfd, monkeypatch, atom, "k_vv_mid fp64, CM removal every step", cm_term=v_cm * DT, proves=proves)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_massless_runner_still_counts(pkg, slack, capfd, monkeypatch, dtype):
    """mass 0: no acceleration (calc_accels), the atom coasts at (2, −1, 0.5); its displacement 10·dt·|v| and its speed are the maxima"""
    case, atom = _runner_fluid(pkg, 9, dtype, "n-1", massless=True)
    def proves(info): assert info["stats"]["n_fused_steps"] == 0, info["stats"]      # k_vv_mid in either precision at this size (the pair pass of 729 atoms does not integrate)
    _check_measured(slack, pkg, case, dtype, VV0(pkg), capfd, monkeypatch, atom, f"massless runner {np.dtype(dtype).name}", proves=proves)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("slot", ["0", "256", "n-1", "wrap"])
def test_lazy_single_list_line(pkg, slack, capfd, monkeypatch, slot, dtype):
    """a context without the dual list (n_filter_passes == 0): one list of radius r_list kept while nobody moved skin/2; refresh measures synchronously with k_max_disp
    (max_disp2_since, 1024-lane blocks) at the cadence step and prints "max disp … since the build of step 0".  The state it reads is the stored one: x_S, and the
    velocity as the fused loop holds it behind the pair pass of step S — the half-step velocity, as in _check_measured, with the same tolerances."""
    monkeypatch.setenv("MOLLYHIP_OUTER_MARGIN_PM", "0")
    case, atom = _runner_fluid(pkg, 9, dtype, slot, wrap=slot == "wrap")
    S_at = case.rebuild_every
    err, info = _debug_run(pkg, case, dtype, VV0(pkg), S_at + 2, capfd, monkeypatch)
    assert info["stats"]["n_filter_passes"] == 0, info["stats"]      # no dual list
    lines = [m for m in LAZY.finditer(err) if int(m.group(1)) == S_at]
    assert len(lines) == 1 and int(lines[0].group(3)) == 0, err
    d, v_max = float(lines[0].group(2)), float(lines[0].group(4))
    states, _ = _quiet_states(pkg, case, dtype, VV0(pkg), (S_at - 1, S_at))
    X0, XS = states[0][0], states[S_at][0]
    if slot == "wrap":
        assert X0[atom, 0] > case.box[0] - 0.01 and XS[atom, 0] < 0.1, (X0[atom], XS[atom])
    d2 = assert_runner(R.disp2(XS, X0, case.box), atom, "lazy single: d(x_S, x_0)")
    v2 = assert_runner((R.minimg(XS - states[S_at - 1][0], case.box) ** 2).sum(axis=1) / DT ** 2, atom, "lazy single: half-step speed")
    L = float(case.box.max())
    print(f"[lazy {slot}] printed d {d} v_max {v_max}; reference {np.sqrt(d2):.9g} {np.sqrt(v2):.9g}")
    slack("lazy single list: printed max disp vs reference, nm", abs(d - np.sqrt(d2)), HALF_D + R.tol_root(R.tol_d2(dtype, L, d2), d2))
    slack("lazy single list: printed v_max vs reference, nm/ps", abs(v_max - np.sqrt(v2)),
          HALF_V + R.tol_root(R.tol_v2(dtype, v2), v2) + np.sqrt(3.0) * 2.0 * R.EPS[np.dtype(dtype)] * L / DT)


def test_vv_mid_fp64_on_a_sheared_face(pkg, slack, capfd, monkeypatch):
    """the plain fp64 VV loop in a TriclinicBoundary (4096 atoms of the suite's sheared fluid, cell grid and dual list): the runner leaves through the sheared +b face
    before the check, and k_vv_mid's written-out tail must take the image through the fractional coordinates — a per-axis image is wrong by b's x component"""
    from tests.test_gpu_triclinic import sheared_fluid
    dtype = np.float64
    basis, case = sheared_fluid(dtype, n_side=16)
    fr = np.linalg.solve(basis.T, case.coords.T).T
    atom = int(np.argmax(fr[:, 1]))
    to_face(case, atom, dtype, basis=basis)
    vel = np.array([2.0, 1.0, 0.5])      # (mirrored in y: towards +b)
    give_runner(case, atom, v=vel)
    def proves(info): assert info["stats"]["n_fused_steps"] == 0 and info["stats"]["minimg_mode"] == 0, info["stats"]
    _check_measured(slack, pkg, case, dtype, VV0(pkg), capfd, monkeypatch, atom, "k_vv_mid fp64 sheared cell", proves=proves, wrapped=True)


# ---- C: mhip_check_finite -----------------------------------------------------------------------------------------------------------------
def _lattice_case(n, dtype):
    """n argon atoms on the first n sites of a 7 × 7 × 7 lattice (0.45 nm apart) in a 3.15 nm box"""
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    x = ((g + 0.5) * 0.45).astype(dtype).astype(np.float64)
    rng = np.random.default_rng(n)
    v = (rng.normal(size=(n, 3)) * 0.13).astype(dtype).astype(np.float64)
    return S.Case(x, 3.15, lj=dict(cutoff=("distance", 1.0)), r_list=1.2, velocities=v, sigma=np.full(n, 0.34), eps=np.full(n, 0.997), mass=np.full(n, 39.948),
                  name=f"lattice{n}")


BAD = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "2e30": 2e30}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_check_finite(pkg, n, dtype):
    """mhip_check_finite (k_check_finite, one lane per owned atom, 256-lane blocks): MHIP_ERR_NAN = −7 "NaN or overflow found in coordinates, velocities or
    forces" for a NaN, an infinity of either sign or a finite magnitude above 1e30 in any of the three arrays; success otherwise, and again after the state
    was mended — the flag does not stick.  The list checks above skip a NaN coordinate silently (fmaxf(m, NaN) == m): this call is the guard.
    (set_state wraps coordinates into the box; a magnitude beyond the guard's bound is stored as given, so that the guard sees it.)"""
    L = pkg.lib()
    case = _lattice_case(n, dtype)
    perm = sorted_order(pkg, case, dtype)
    s = case.system(pkg, dtype)
    ctx = s.engine()
    x0 = np.ascontiguousarray(case.coords, dtype=dtype); v0 = np.ascontiguousarray(case.velocities, dtype=dtype)

    def state(x, v):
        s._check(L.mhip_set_state(ctx, s._ptr(x), s._ptr(v), HOST))

    try:
        state(x0, v0)
        f = np.zeros((n, 3), dtype)
        s._check(L.mhip_forces(ctx, 0, 0, s._ptr(f), None, HOST))
        assert np.isfinite(f).all()
        assert L.mhip_check_finite(ctx) == 0
        for atom in sorted({int(perm[0]), int(perm[n - 1])}):
            for name, bad in BAD.items():
                for arr in ("coords", "velocities"):
                    x, v = x0.copy(), v0.copy()
                    (x if arr == "coords" else v)[atom, 1] = bad
                    state(x, v)
                    rc = L.mhip_check_finite(ctx)
                    assert rc == ERR_NAN, f"{name} in the {arr} of atom {atom}: status {rc}"
                    with pytest.raises(pkg.MollyHipError) as ei:
                        s._check(rc)
                    assert ei.value.code == ERR_NAN and "NaN or overflow" in str(ei.value)
                    state(x0, v0)
                    assert L.mhip_check_finite(ctx) == 0, f"the flag stuck after {name} in the {arr}"
        # every component on its own: +2e30 and −2e30 in one atom's velocity do not cancel, and components that are each in range do not add up to an alarm
        a = int(perm[n - 1])
        v = v0.copy(); v[a] = (2e30, -2e30, 0.0)
        state(x0, v)
        assert L.mhip_check_finite(ctx) == ERR_NAN
        v = v0.copy(); v[a] = (4e29, 4e29, 4e29)
        state(x0, v)
        assert L.mhip_check_finite(ctx) == 0
        state(x0, v0)
        assert L.mhip_check_finite(ctx) == 0
    finally:
        s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_check_finite_sees_a_force(pkg, dtype):
    """two atoms on top of each other: r = 0, the Lennard-Jones force is inf − inf; the force array is checked as well, and simulate(check_nans=True) raises"""
    L = pkg.lib()
    n = 65
    case = _lattice_case(n, dtype)
    perm = sorted_order(pkg, case, dtype)
    a, b = int(perm[n - 1]), int(perm[0])
    x = case.coords.copy(); x[a] = x[b]
    s = case.system(pkg, dtype, coords=x)
    try:
        f = pkg.forces(s)
        assert not np.isfinite(f[[a, b]]).all()
        assert L.mhip_check_finite(s.engine()) == ERR_NAN
        s.coords[:] = np.ascontiguousarray(case.coords, dtype=dtype)
        f = pkg.forces(s)
        assert np.isfinite(f).all() and L.mhip_check_finite(s.engine()) == 0
        s.coords[:] = np.ascontiguousarray(x, dtype=dtype)
        with pytest.raises(pkg.MollyHipError) as ei:
            pkg.simulate(s, pkg.VelocityVerlet(dt=DT, remove_CM_motion=0), 2, check_nans=True)
        assert ei.value.code == ERR_NAN
    finally:
        s.close()


# ---- B, continued: the prune line, constraints, bonded + PME, the synchronous loops ----------------------------------------------------------
STEP_LINE = re.compile(r"\[mhip\] step (\d+):")


PRUNE_CASES = {   # fluid, precision, check interval, time step, steps run, the pass that prunes
    "lj_fp32_packed": ("lj", np.float32, 4, DT, 14),
    "lj_fp64": ("lj", np.float64, 4, DT, 14),
    "charged_fp32": ("charged", np.float32, 4, DT, 14),
}


def _prune_fluid(pkg, kind, dtype, every, wrap):
    """The inner skin sized at the search (three check intervals of the runner's drift) is used up by the runner within the run, the outer margin is not.
    lj: 21³ atoms, the size at which the fp32 pair pass is the packed one (STEP_SIDE).  charged: the argon fluid of 13³ atoms with charges of ±0.1 e in turn (the last
    atom neutral: no net charge) under CoulombReactionField — the Lennard-Jones cores keep it as calm as the plain fluid, which the suite's charged_fluid with its
    free hydrogens of mass 1 (20 to 30 nm/ps within a few dozen steps) is not."""
    if kind == "charged":
        fl = S.lj_fluid(13, dtype=dtype, rebuild_every=every)
        q = np.where(np.arange(fl.n) % 2 == 0, 0.1, -0.1); q[-1] = 0.0
        case = S.Case(fl.coords, fl.box, lj=fl.lj, coul=dict(kind="rf", rc=1.0), r_list=fl.r_list, rebuild_every=every, velocities=fl.velocities, charge=q,
                      sigma=fl.sigma, eps=fl.eps, mass=fl.mass, name="lj2197_charged")
    else:
        case = S.lj_fluid(STEP_SIDE[64], dtype=dtype, rebuild_every=every)
    if wrap:
        atom = int(np.argmax(case.coords[:, 0]))
        to_face(case, atom, dtype)
    else:
        atom = int(sorted_order(pkg, case, dtype)[case.n - 1])
    return give_runner(case, atom), atom


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("name", sorted(PRUNE_CASES))
def test_prune_line_displacement_since_the_search(pkg, slack, capfd, monkeypatch, name, wrap):
    """blk_disp2 of the pruning passes → k_prune_summary: the largest displacement since the outer search, taken while pruning.  Three passes: the packed emitter
    of the fp32 one-type fluid (shown by n_fused_steps > 0: only the packed pass integrates), and k_forces' generic pruning pass in fp64 and for a charged fluid
    (n_fused_steps == 0: a pass with double precision or a Coulomb term is never the packed one).  The policy prunes inside the run (stats: one search, and as many
    prunes as prune lines, the one of step 0 among them); the first prune inside the run is compared.  It runs in the force pass of the step p at which it was
    decided — the last "step p:" line in front of the second prune line — at the coordinates x_p, which a quiet context stopped after p steps holds.  wrap: the
    runner has crossed the +x face by then.  Tolerance: half a unit of the printed %.5f nm plus the bound of A at the root."""
    kind, dtype, every, dt, n_steps = PRUNE_CASES[name]
    case, atom = _prune_fluid(pkg, kind, dtype, every, wrap)
    sim = pkg.VelocityVerlet(dt=dt, remove_CM_motion=0)
    err, info = _debug_run(pkg, case, dtype, sim, n_steps, capfd, monkeypatch)
    st = info["stats"]
    assert (st["n_fused_steps"] > 0) == (name == "lj_fp32_packed"), st
    prunes = list(PRUNE.finditer(err))
    assert st["n_outer_builds"] == 1 and st["n_filter_passes"] == len(prunes) >= 2, (st, err)
    assert float(prunes[0].group(1)) == 0.0                       # the prune of step 0: nobody has moved
    steps = [int(m.group(1)) for m in STEP_LINE.finditer(err[:prunes[1].start()])]
    assert steps, err
    p = steps[-1]
    states, _ = _quiet_states(pkg, case, dtype, sim, (p,))
    X0, Xp = states[0][0], states[p][0]
    if wrap:
        assert X0[atom, 0] > case.box[0] - 0.01 and Xp[atom, 0] < 0.1, (X0[atom], Xp[atom])
    d2 = assert_runner(R.disp2(Xp, X0, case.box), atom, f"prune at step {p}: d(x_p, x_0)")
    L = float(case.box.max())
    printed = float(prunes[1].group(1))
    print(f"[prune {name} wrap {wrap}] step {p}: printed {printed}, reference {np.sqrt(d2):.9g}")
    slack(f"prune line ({name}): displacement since the search vs reference, nm", abs(printed - np.sqrt(d2)), HALF_D + R.tol_root(R.tol_d2(dtype, L, d2), d2))


CON_DT = 0.001


def _constrained_case():
    """tests/constraints_ref.toy_system on 5³ cells (3 nm box: room for the outer margin, so the dual list and the measuring launches) — every cluster kind 31 times —
    at a tenth of its velocities, plus ONE free argon-like atom on a cell corner (0.5 nm from every cluster centre) as the runner: k_con_step carries free atoms
    as work items of their own (CK_FREE), behind the last cluster.  The hydrogens (mass 1) are driven to 1.8 nm/ps by the forces within a few steps whatever they start
    with: the runner gets twice its usual velocity and the run half the usual time step (CON_DT), which leaves its displacement per interval where it was."""
    from tests import constraints_ref as CR
    t = CR.toy_system(n_side=5)
    n = t.n
    cat = lambda a, v: np.concatenate([np.asarray(a, np.float64), [v]])
    case = S.Case(np.vstack([t.coords, [[1.2, 1.2, 1.2]]]), t.box, lj=t.lj, coul=t.coul, r_list=t.r_list, rebuild_every=t.rebuild_every,
                  velocities=np.vstack([0.1 * t.velocities, [2.0 * RUNNER_V]]), charge=cat(t.charge, 0.0), sigma=cat(t.sigma, 0.3), eps=cat(t.eps, 0.4),
                  mass=cat(t.mass, 39.948), excluded=t.excluded, name="constraint_toy_runner", constraints=dict(t.constraints, dist_tolerance=1e-10))
    return case, n


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("form", ["vv", "langevin", "thermostat"])
def test_con_step_measures(pkg, slack, capfd, monkeypatch, form, wrap):
    """k_con_step: mode 1 between the force passes of constrained velocity Verlet, mode 3 of constrained Langevin, and the thermostat's close (2) – open (0) pair.
    constraint_info shows the clusters and that SHAKE iterated in the run; thermostat_info that the coupling applied on every step.  The kernel walks work items
    (clusters by kind, then the free atoms), not sorted slots: the runner is the one free item, the last of the launch.  wrap: the whole system is shifted so that
    the runner starts 0.005 nm inside the +x face and is wrapped before the check."""
    dtype = np.float64
    case, atom = _constrained_case()
    if wrap:
        to_face(case, atom, dtype)
    rng = None
    if form == "vv":
        sim = pkg.VelocityVerlet(dt=CON_DT, remove_CM_motion=0)
    elif form == "langevin":
        sim, rng = pkg.Langevin(dt=CON_DT, temperature=3.0, friction=1.0, remove_CM_motion=0), 9
    else:
        s = case.system(pkg, dtype); T0 = pkg.temperature(s); s.close()      # the system's own temperature: λ ≈ 1, the runner keeps its speed
        sim = pkg.VelocityVerlet(dt=CON_DT, remove_CM_motion=0, coupling=pkg.ImmediateThermostat(temperature=T0))
    n_run = case.rebuild_every + 2

    def proves(info):
        c = info["constraints"]
        assert c["clusters12"] > 0 and c["angle_clusters"] > 0 and c["max_iters_last_run"] >= 1 and c["n_not_converged"] == 0, c
        assert info["stats"]["n_fused_steps"] == 0
        if form == "thermostat":
            assert info["thermostat"]["n_applied"] == n_run, info["thermostat"]
    _check_measured(slack, pkg, case, dtype, sim, capfd, monkeypatch, atom, f"k_con_step {form} wrap {wrap}", rng=rng, half_step_v=form != "langevin", proves=proves, dt=CON_DT, wrapped=wrap)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("form", ["vv", "langevin"])
def test_gather_collect_integrating_launch_measures(pkg, slack, capfd, monkeypatch, form, wrap):
    """the integrating gather–collect launch of step_fused.h on the suite's smallest bonded + PME fixture (tests/bonded_ref.fluid_with_chains, fp32, its own time
    step): n_group_split_passes > 0 and n_fused_steps > 0 as in test_gpu_bonded's launch shapes.  The fluid atoms get the fluid's velocities, one of them runs."""
    from tests import bonded_ref as BR
    monkeypatch.delenv("MOLLYHIP_GROUP_SPLIT", raising=False)
    monkeypatch.setenv("MOLLYHIP_FUSE_GATHER_VV", "1")
    dtype = np.float32
    case = BR.fluid_with_chains("pme")
    case.velocities = np.vstack([S.lj_fluid(12, dtype=dtype).velocities, np.zeros((case.n - case.n_fluid, 3))])
    if wrap:      # the fluid atom nearest the +x face, everything shifted so that it starts 0.005 nm inside it
        atom = int(np.argmax(case.coords[:case.n_fluid, 0]))
        to_face(case, atom, dtype)
    else:
        perm = sorted_order(pkg, case, dtype)
        atom = int(next(a for a in perm[::-1] if a < case.n_fluid))      # the last sorted slot that holds a fluid atom
    give_runner(case, atom, v=3.0 * RUNNER_V)      # (the chains start away from rest lengths: their atoms reach 3 nm/ps and move 0.008 nm in ten steps)
    if form == "vv":
        sim, rng = pkg.VelocityVerlet(dt=BR.RUN_DT, remove_CM_motion=0), None
    else:
        sim, rng = pkg.Langevin(dt=BR.RUN_DT, temperature=85.0, friction=1.0, remove_CM_motion=0), 13

    def proves(info):
        assert info["stats"]["n_group_split_passes"] > 0 and info["stats"]["n_fused_steps"] > 0, info["stats"]
    _check_measured(slack, pkg, case, dtype, sim, capfd, monkeypatch, atom, f"gather-collect {form} wrap {wrap}", rng=rng, half_step_v=form == "vv", proves=proves, dt=BR.RUN_DT, wrapped=wrap)


def test_splitting_loop_leaves_what_the_direct_call_measures(pkg, slack):
    """mhip_splitting_run measures synchronously (refresh → k_max_disp) and prints no line of its own; checked through A's direct call right behind a run of 8
    steps (no cadence step inside: the stats show the search and the prune of step 0 only, both snapshots are the wrapped start): the triple is
    {d²(x_8, x_0), the same, |v_8|²} of the state the run left."""
    dtype = np.float64
    case, atom = _runner_fluid(pkg, 9, dtype, "n-1")
    L_ = pkg.lib()
    s = case.system(pkg, dtype)
    try:
        s.push_state(); s.pull_state()
        X0 = s.coords.astype(np.float64)
        pkg.simulate(s, pkg.LangevinSplitting(dt=DT, temperature=85.0, friction=0.1, splitting="BAOAB", remove_CM_motion=0), 8, rng=5)
        st = s.stats()
        out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s._check(L_.mhip_plan_state_dev(s.engine(), C.c_void_p(out3.data_ptr())))
        s._check(L_.mhip_synchronize(s.engine()))
        torch.cuda.synchronize()
        got = out3.cpu().numpy().astype(np.float64)
        X8, V8 = s.coords.astype(np.float64), s.velocities.astype(np.float64)
    finally:
        s.close()
    assert (st["n_outer_builds"], st["n_filter_passes"]) == (1, 1), st
    d2 = assert_runner(R.disp2(X8, X0, case.box), atom, "splitting: d(x_8, x_0)")
    v2 = assert_runner(R.speed2(V8), atom, "splitting: |v_8|")
    L = float(case.box.max())
    print(f"[splitting] plan_state_dev {got}, reference {d2} {v2}")
    slack("splitting run: max |x - x_search|^2 vs reference", abs(got[0] - d2), R.tol_d2(dtype, L, d2))
    slack("splitting run: max |x - x_prune|^2 vs reference", abs(got[1] - d2), R.tol_d2(dtype, L, d2))
    slack("splitting run: max |v|^2 vs reference", abs(got[2] - v2), R.tol_v2(dtype, v2))


def test_overdamped_loop_leaves_what_the_direct_call_measures(pkg, slack):
    """mhip_overdamped_run: positions move by F·dt/(γ m) and a noise of variance 2 kT dt/(γ m) per axis; velocities take no part.  The runner here is a LIGHT atom
    (a hundredth of the mass: ten times the noise, a hundred times the drift) that also carries the runner's velocity in the stored state.  Three steps, no cadence
    step inside (stats: the search and the prune of step 0 only), then A's direct call against {d²(x_3, x_0), the same, |v|² of the state the run left}."""
    dtype = np.float64
    case, atom = _runner_fluid(pkg, 9, dtype, "n-1")
    case.mass = case.mass.copy(); case.mass[atom] /= 100.0
    L_ = pkg.lib()
    s = case.system(pkg, dtype)
    try:
        s.push_state(); s.pull_state()
        X0 = s.coords.astype(np.float64)
        pkg.simulate(s, pkg.OverdampedLangevin(dt=DT, temperature=85.0, friction=10.0, remove_CM_motion=0), 3, rng=5)
        st = s.stats()
        out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s._check(L_.mhip_plan_state_dev(s.engine(), C.c_void_p(out3.data_ptr())))
        s._check(L_.mhip_synchronize(s.engine()))
        torch.cuda.synchronize()
        got = out3.cpu().numpy().astype(np.float64)
        X3, V3 = s.coords.astype(np.float64), s.velocities.astype(np.float64)
    finally:
        s.close()
    assert (st["n_outer_builds"], st["n_filter_passes"]) == (1, 1), st
    d2 = assert_runner(R.disp2(X3, X0, case.box), atom, "overdamped: d(x_3, x_0)")
    v2 = assert_runner(R.speed2(V3), atom, "overdamped: |v| as stored")
    L = float(case.box.max())
    print(f"[overdamped] plan_state_dev {got}, reference {d2} {v2}")
    slack("overdamped run: max |x - x_search|^2 vs reference", abs(got[0] - d2), R.tol_d2(dtype, L, d2))
    slack("overdamped run: max |x - x_prune|^2 vs reference", abs(got[1] - d2), R.tol_d2(dtype, L, d2))
    slack("overdamped run: max |v|^2 vs reference", abs(got[2] - v2), R.tol_v2(dtype, v2))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plan_state_runs_over_owned_atoms_only(pkg, slack, dtype):
    """A single-rank context with ghosts (mhip_set_ghost_margin, then mhip_set_atom_counts: the last 40 atoms of the fluid in caller order become ghosts; no halo
    exchange, no second rank).  mhip_plan_state_dev measures the OWNED atoms only — every ghost is some rank's owned atom, and its velocity never reaches this
    context: mhip_set_state takes n_owned velocity rows.  An owned runner moves 0.012 nm and runs at (2, −1, 0.5); a ghost is handed over 0.03 nm away, and the
    velocity rows behind n_owned are not the caller's to set (the ghost was handed over at (5, 5, 5) while it was still owned: whatever is left of that must not count).  The triple must be the owned runner's
    {0.012², 0.012², 5.25}; mhip_plan_disp2_dev, which vouches for the ghost plan, covers the ghosts too and reports the ghost's 0.03² for both snapshots."""
    L_ = pkg.lib()
    case = S.lj_fluid(9, dtype=dtype)
    n, k = case.n, 40
    n_owned = n - k
    perm = sorted_order(pkg, case, dtype)
    atom = int(next(a for a in perm[::-1] if a < n_owned))
    ghost = n - 1
    s = case.system(pkg, dtype)
    try:
        ctx = s.engine()
        v_all = np.ascontiguousarray(case.velocities, dtype=dtype); v_all[ghost] = (5.0, 5.0, 5.0)
        x0 = np.ascontiguousarray(case.coords, dtype=dtype)
        s._check(L_.mhip_set_state(ctx, s._ptr(x0), s._ptr(v_all), HOST))              # all owned still: the future ghost's row is fast
        s._check(L_.mhip_set_ghost_margin(ctx, 0.2))
        s._check(L_.mhip_set_atom_counts(ctx, n_owned, k))
        s._push_atoms()
        v_own = np.ascontiguousarray(case.velocities[:n_owned], dtype=dtype)
        s._check(L_.mhip_set_state(ctx, s._ptr(x0), s._ptr(v_own), HOST))
        f = np.zeros((n, 3), dtype)
        s._check(L_.mhip_forces(ctx, 0, 0, s._ptr(f), None, HOST))
        st = s.stats()
        assert (st["n_owned"], st["n_ghost"]) == (n_owned, k) and (st["n_outer_builds"], st["n_filter_passes"]) == (1, 1), st
        X0 = np.empty((n, 3), dtype)
        s._check(L_.mhip_get_state(ctx, s._ptr(X0), None, HOST))
        X0 = X0.astype(np.float64)
        x1 = X0.copy(); x1[atom] += 0.012 * RUNNER_U; x1[ghost] += 0.03 * RUNNER_U
        x1 = np.ascontiguousarray(x1, dtype=dtype)
        v1 = np.ascontiguousarray(give_vel(case.velocities, atom)[:n_owned], dtype=dtype)
        s._check(L_.mhip_set_state(ctx, s._ptr(x1), s._ptr(v1), HOST))
        X1 = np.empty((n, 3), dtype); V1 = np.empty((n_owned, 3), dtype)
        s._check(L_.mhip_get_state(ctx, s._ptr(X1), s._ptr(V1), HOST))
        X1, V1 = X1.astype(np.float64), V1.astype(np.float64)
        out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
        out2 = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s._check(L_.mhip_plan_state_dev(ctx, C.c_void_p(out3.data_ptr())))
        s._check(L_.mhip_plan_disp2_dev(ctx, C.c_void_p(out2.data_ptr())))
        s._check(L_.mhip_synchronize(ctx))
        torch.cuda.synchronize()
        got3, got2 = out3.cpu().numpy().astype(np.float64), out2.cpu().numpy().astype(np.float64)
    finally:
        s.close()
    a_d = R.disp2(X1, X0, case.box)
    d_own = assert_runner(a_d[:n_owned], atom, "owned atoms: d(X1, X0)")
    d_all = assert_runner(a_d, ghost, "all atoms: d(X1, X0)")
    v_ownd = assert_runner(R.speed2(V1, n_owned), atom, "owned atoms: |V1|")
    L = float(case.box.max())
    print(f"[owned only] plan_state_dev {got3}, plan_disp2_dev {got2}; owned {d_own} all {d_all} v2 {v_ownd}")
    for k_ in range(2):
        slack(f"ghosted context: plan_state_dev entry {k_} is the owned runner's", abs(got3[k_] - d_own), R.tol_d2(dtype, L, d_own))
        slack(f"ghosted context: plan_disp2_dev entry {k_} is the ghost's", abs(got2[k_] - d_all), R.tol_d2(dtype, L, d_all))
    slack("ghosted context: max |v|^2 over the owned atoms", abs(got3[2] - v_ownd), R.tol_v2(dtype, v_ownd))
