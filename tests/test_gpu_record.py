"""The recorder (csrc/record.h, record_plan.h; mhip_set_record, mhip_record_now, mhip_record_info, mhip_record_read, mhip_record_clear) inside the device step
loops, through the C ABI.  The yardstick throughout uses none of the recorder's code: the same run on a fresh context of the same case, cut into chunks at
the union of the record steps through mhip_vv_run / mhip_langevin_run, and behind each chunk — in this fixed order, only for the channels due at that step —
mhip_kinetic_energy, the three potential-energy entry points, mhip_get_state.  A record step is a chunk boundary without the host, so every comparison is
`==` on the raw bytes; only the PME route, whose mesh is filled with float atomics, repeats to rounding and has a measured bar."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import admit_walk
from tests import systems as S
from tests.test_gpu_thermostat import fluid, route, truncated      # noqa: F401  (the thermostat tests' systems)

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED = 0, -1, -4, -6
KE, PE, X, V = 0, 1, 2, 3
KB = 8.314462618e-3
KEY, CTR1 = 0x1234567890ABCDEF, 0x0FEDCBA987654321
EVERY = (3, 6, 5, 10)      # with a rebuild cadence of 10 and 25 steps: records at cadence steps (10, 20) and at the run's last step (25, coordinates)

p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the systems -----------------------------------------------------------------------------------------------------------------------------
_cases = {}


def case_of(name):
    """→ (case, dt, cm of the route).  edgeN: the first N atoms of a one-type fluid (343 atoms hold the sizes up to 257; 513 — three blocks, ragged — is cut
    from the 729-atom fluid of the same recipe); packed: the untruncated fp32 fluid of 21³ atoms, the smallest of the suite whose pair pass is the packed one
    and integrates (n_fused_steps > 0; tests/test_gpu_list_checks.py STEP_SIDE — the pass of the 343-atom fluid never does); the rest: the routes of
    tests/test_gpu_thermostat.py"""
    if name not in _cases:
        if name.startswith("edge"):
            n = int(name[4:])
            _cases[name] = (truncated(S.lj_fluid(7 if n <= 343 else 9, seed=3), n), 0.002, 1)
        elif name == "packed":
            _cases[name] = (S.lj_fluid(21, seed=3, dtype=np.float32), 0.002, 1)
        elif name == "small32":      # the `small` route with its inputs rounded to fp32: the gather-collect launch integrates (k_gather_collect_vv)
            from tests import golden6mrr as G
            _cases[name] = (G.case("ewald", np.float32, bonded=True, pme=True), 0.0005, 1)
        else:
            r = route(name)
            _cases[name] = (r["case"], r["dt"], r["cm"])
    return _cases[name]


def fresh(pkg, name, dtype):
    s = case_of(name)[0].system(pkg, dtype)
    s.push_state(velocities=True)
    return s


# ---- the ABI, with the status checked ----------------------------------------------------------------------------------------------------------
def ok(L, s, rc):
    assert rc == OK, (rc, L.mhip_last_error(s._ctx).decode())


def set_record(L, s, every, capacity):
    return L.mhip_set_record(s._ctx, C.byref((C.c_int32 * 4)(*every)), C.byref((C.c_int64 * 4)(*capacity)))


def info_of(L, s):
    out = (C.c_int64 * 16)()
    ok(L, s, L.mhip_record_info(s._ctx, C.byref(out)))
    return [list(out[4 * c: 4 * c + 4]) for c in range(4)]


def width(c, s):
    return (1, 3, 3 * len(s), 3 * len(s))[c]


def read_channel(L, s, c):
    """→ (steps, values as an (n, width) array of the channel's type)"""
    n = info_of(L, s)[c][2]
    steps = np.full(n, -7, np.int64)
    vals = np.zeros((n, width(c, s)), np.float64 if c < X else s.dtype)
    if n:
        ok(L, s, L.mhip_record_read(s._ctx, c, 0, n, p(steps), p(vals), 0))
    return steps, vals


def capacities(every, first, n, extra=0):
    return [((first + n) // e - first // e + extra) if e else 0 for e in every]


def run_call(L, s, kind, first, n, dt, cm, first0):
    if kind == "vv":
        return L.mhip_vv_run(s._ctx, first, n, dt, cm)
    return L.mhip_langevin_run(s._ctx, first, n, dt, KB * 120.0, 2.0, cm, KEY, (CTR1 + (first - first0)) % 2 ** 64)      # ctr1 advances by one per step, as api.py's simulate passes it


def host_reads(L, s, step, mask):
    """the existing entry points, in the yardstick's fixed order → {channel: bytes of one record}"""
    out, d = {}, C.c_double(0)
    if mask & (1 << KE):
        ok(L, s, L.mhip_kinetic_energy(s._ctx, C.byref(d)))
        out[KE] = np.array([d.value]).tobytes()
    if mask & (1 << PE):
        e = []
        for call in (lambda: L.mhip_potential_energy(s._ctx, step, C.byref(d)), lambda: L.mhip_specific_potential_energy(s._ctx, C.byref(d)),
                     lambda: L.mhip_general_potential_energy(s._ctx, C.byref(d))):
            ok(L, s, call())
            e.append(d.value)
        out[PE] = np.array(e).tobytes()
    if mask & ((1 << X) | (1 << V)):
        x = np.zeros((len(s), 3), s.dtype) if mask & (1 << X) else None
        v = np.zeros((len(s), 3), s.dtype) if mask & (1 << V) else None
        ok(L, s, L.mhip_get_state(s._ctx, p(x), p(v), 0))
        if x is not None:
            out[X] = x.tobytes()
        if v is not None:
            out[V] = v.tobytes()
    return out


def mask_at(every, step):
    return sum(1 << c for c in range(4) if every[c] and step % every[c] == 0)


def final_state(L, s):
    s.pull_state()
    return s.coords.tobytes(), s.velocities.tobytes()


def yardstick(pkg, name, dtype, every, runs, kind="vv", cm=None, setup=None, profiling=False):
    """the run cut at the union of the record steps → ({channel: [(step, bytes)]}, final state, stats)"""
    L = pkg.lib()
    _, dt, cm0 = case_of(name)
    cm = cm0 if cm is None else cm
    s = fresh(pkg, name, dtype)
    if profiling:
        ok(L, s, L.mhip_set_profiling(s._ctx, 1))
    if setup:
        setup(L, s)
    hist = {c: [] for c in range(4)}
    first0 = runs[0][0]
    for first, n in runs:
        at = first
        stops = [st for st in range(first + 1, first + n + 1) if mask_at(every, st)]
        for stop in stops + ([first + n] if first + n not in stops else []):
            ok(L, s, run_call(L, s, kind, at, stop - at, dt, cm, first0))
            for c, b in host_reads(L, s, stop, mask_at(every, stop)).items():
                hist[c].append((stop, b))
            at = stop
    stats = s.stats()
    return hist, final_state(L, s), stats


def recorded(pkg, name, dtype, every, runs, kind="vv", cm=None, setup=None, profiling=False):
    """the same run with the recorder on → the same three things, and the System"""
    L = pkg.lib()
    _, dt, cm0 = case_of(name)
    cm = cm0 if cm is None else cm
    s = fresh(pkg, name, dtype)
    if profiling:
        ok(L, s, L.mhip_set_profiling(s._ctx, 1))
    if setup:
        setup(L, s)
    total = [sum(x) for x in zip(*[capacities(every, f, n) for f, n in runs])]
    ok(L, s, set_record(L, s, every, [max(t, 1) if e else 0 for t, e in zip(total, every)]))
    for first, n in runs:
        ok(L, s, run_call(L, s, kind, first, n, dt, cm, runs[0][0]))
    hist = {}
    for c in range(4):
        steps, vals = read_channel(L, s, c) if every[c] else ([], [])
        hist[c] = [(int(st), v.tobytes()) for st, v in zip(steps, vals)]
    stats = s.stats()
    return hist, final_state(L, s), stats, s


def plain_run(pkg, name, dtype, runs, kind="vv", cm=None, setup=None, profiling=False):
    """uncut and unrecorded, on a context that never had a recorder"""
    return yardstick(pkg, name, dtype, (0, 0, 0, 0), runs, kind, cm, setup, profiling)


def assert_same_history(got, want):
    for c in range(4):
        assert [st for st, _ in got[c]] == [st for st, _ in want[c]], (c, [st for st, _ in got[c]], [st for st, _ in want[c]])
        for (st, a), (_, b) in zip(got[c], want[c]):
            assert a == b, f"channel {c}, step {st}: the record differs from the yardstick's"


# ---- 1. mhip_record_now at the block edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_record_now_equals_the_entry_points_at_the_block_edges(pkg, n, dtype):
    import torch
    L = pkg.lib()
    name = f"edge{n}"
    s = fresh(pkg, name, dtype)
    assert len(s) == n
    d = C.c_double(0)
    ok(L, s, L.mhip_potential_energy(s._ctx, 0, C.byref(d)))      # the first search sorts the atoms: both readers of step 0 then sum the kinetic energy in one order
    ok(L, s, set_record(L, s, [1000] * 4, [2] * 4))      # (intervals the 3-step run does not reach: both records are mhip_record_now's)
    ok(L, s, L.mhip_record_now(s._ctx, 0, 15))
    want = [host_reads(L, s, 0, 15)]
    ok(L, s, L.mhip_vv_run(s._ctx, 0, 3, 0.002, 1))      # remove_CM_motion = 1
    ok(L, s, L.mhip_record_now(s._ctx, 3, 15))
    want.append(host_reads(L, s, 3, 15))
    assert [r[2:] for r in info_of(L, s)] == [[2, 3]] * 4
    for c in range(4):
        steps, vals = read_channel(L, s, c)
        assert steps.tolist() == [0, 3]
        for k in range(2):
            assert vals[k].tobytes() == want[k][c], (c, k, vals[k][:6], np.frombuffer(want[k][c], vals.dtype)[:6])
        dev = torch.zeros(vals.size, dtype=torch.float64 if c < X else (torch.float32 if dtype == np.float32 else torch.float64), device="cuda")
        torch.cuda.synchronize()      # (the fill runs on torch's stream, the copy on the context's)
        ok(L, s, L.mhip_record_read(s._ctx, c, 0, 2, None, C.c_void_p(dev.data_ptr()), 1))
        ok(L, s, L.mhip_synchronize(s._ctx))
        assert dev.cpu().numpy().tobytes() == vals.tobytes(), c
    assert np.frombuffer(want[1][KE])[0] > 0 or n == 1      # (one atom: the removal leaves it at rest)


# ---- 2., 3. in-run records of both loops ---------------------------------------------------------------------------------------------------------
VV_CASES = [("edge257", np.float64), ("edge257", np.float32), ("packed", np.float32), ("constrained", np.float64), ("sites", np.float64)]
LANGEVIN_CASES = [("edge257", np.float64), ("edge257", np.float32), ("packed", np.float32), ("constrained", np.float64)]
ids = lambda cases: [f"{n}-{np.dtype(d).name}" for n, d in cases]


def in_run(pkg, name, dtype, kind, cm):
    want, end_want, st_want = yardstick(pkg, name, dtype, EVERY, [(0, 25)], kind, cm)
    got, end_got, st_got, _ = recorded(pkg, name, dtype, EVERY, [(0, 25)], kind, cm)
    assert [len(got[c]) for c in range(4)] == [8, 4, 5, 2]
    assert_same_history(got, want)
    assert end_got == end_want, "the final state differs from the yardstick's"
    if cm == 0:
        _, end_plain, _ = plain_run(pkg, name, dtype, [(0, 25)], kind, cm)
        assert end_got == end_plain, "the final state differs from the uncut, unrecorded run's"
    return st_got, st_want


@pytest.mark.parametrize("cm", [0, 1])
@pytest.mark.parametrize("name,dtype", VV_CASES, ids=ids(VV_CASES))
def test_records_inside_the_velocity_verlet_loop(pkg, name, dtype, cm):
    """plain: k_vv_mid; packed: the pair pass integrates; constrained, sites: k_con_step (the thermostat tests' routes, fp64 as there: their solver tolerances are
    fp64 settings).  cm: remove_CM_motion — every step or never."""
    in_run(pkg, name, dtype, "vv", cm)


@pytest.mark.parametrize("cm", [0, 1])
@pytest.mark.parametrize("name,dtype", LANGEVIN_CASES, ids=ids(LANGEVIN_CASES))
def test_records_inside_the_langevin_loop(pkg, name, dtype, cm):
    in_run(pkg, name, dtype, "langevin", cm)


# ---- 4. couplings -------------------------------------------------------------------------------------------------------------------------------
def coupling(kind, dof):
    if kind == "berendsen":
        return lambda L, s: ok(L, s, L.mhip_set_thermostat(s._ctx, 2, KB * 300.0, 0.1, 1, dof, KEY, CTR1))
    if kind == "csvr4":
        return lambda L, s: ok(L, s, L.mhip_set_thermostat(s._ctx, 3, KB * 300.0, 0.1, 4, dof, KEY, CTR1))
    return lambda L, s: ok(L, s, L.mhip_set_andersen(s._ctx, KB * 120.0, 0.05, KEY))      # the two-launch form


@pytest.mark.parametrize("name,kind", [("edge257", "berendsen"), ("edge257", "csvr4"), ("constrained", "berendsen"), ("constrained", "csvr4"), ("edge257", "andersen")])
def test_records_of_coupled_runs(pkg, name, kind):
    s0 = case_of(name)[0].system(pkg, np.float64)
    setup = coupling(kind, 3 * (len(s0) - len(s0.virtual_sites)) - 3 - s0.n_constraints)
    want, end_want, _ = yardstick(pkg, name, np.float64, (4, 4, 4, 4), [(0, 20)], setup=setup)
    got, end_got, _, _ = recorded(pkg, name, np.float64, (4, 4, 4, 4), [(0, 20)], setup=setup)
    assert [len(got[c]) for c in range(4)] == [5] * 4
    assert_same_history(got, want)
    assert end_got == end_want


# ---- 5. the PME route ----------------------------------------------------------------------------------------------------------------------------
# The largest deviation between two runs of the yardstick itself, each on a fresh context (bonded terms + PME, fp64, 10 steps, KE every 2, PE every 5), measured
# on an MI355X: relative for the energies (kinetic; pairwise, specific, general), absolute for the final state (nm, nm/ps).  The largest over the six pairs of four
# runs and the pair of this test's own first run.  fp64: the yardstick repeated exactly in every pair, and the bar is ==.  fp32, whose gather-collect launch
# integrates and whose mesh is filled with float atomics: repeats agree to rounding only, amplified over ten steps.  DESIGN §10i has the figures.
PME_REPEAT = {np.float64: {"ke": 0.0, "pe": 0.0, "x": 0.0, "v": 0.0},
              np.float32: {"ke": 3.1416695952842154e-08, "pe": 5.188987680013308e-09, "x": 4.76837158203125e-07, "v": 0.0003682374954223633}}


def pme_deviation(a, b, end_a, end_b, dtype):
    """→ dict of the largest deviations between two (history, final state) pairs"""
    rel = lambda u, w: float(np.max(np.abs(u - w) / np.maximum(np.abs(w), 1e-300))) if len(u) else 0.0
    flat = lambda h, c: np.concatenate([np.frombuffer(r, np.float64) for _, r in h[c]]) if h[c] else np.zeros(0)
    x = lambda e: np.frombuffer(e[0], dtype).astype(np.float64)
    v = lambda e: np.frombuffer(e[1], dtype).astype(np.float64)
    return {"ke": rel(flat(a, KE), flat(b, KE)), "pe": rel(flat(a, PE), flat(b, PE)), "x": float(np.abs(x(end_a) - x(end_b)).max()), "v": float(np.abs(v(end_a) - v(end_b)).max())}


@pytest.mark.parametrize("name,dtype", [("small", np.float64), ("small32", np.float32)], ids=["float64", "float32"])
def test_records_on_the_pme_route(pkg, name, dtype):
    every, runs = (2, 5, 0, 0), [(0, 10)]
    y1, end1, st1 = yardstick(pkg, name, dtype, every, runs)
    y2, end2, _ = yardstick(pkg, name, dtype, every, runs)
    got, end_got, st_got, _ = recorded(pkg, name, dtype, every, runs)
    assert [st for st, _ in got[KE]] == [2, 4, 6, 8, 10] and [st for st, _ in got[PE]] == [5, 10]
    assert all(np.frombuffer(r, np.float64)[2] != 0 and np.frombuffer(r, np.float64)[1] != 0 for _, r in got[PE])      # specific and general terms are there
    print("launches that integrated:", st_got["n_fused_steps"], "recorded,", st1["n_fused_steps"], "yardstick")
    assert st_got["n_fused_steps"] == st1["n_fused_steps"]
    repeat = pme_deviation(y1, y2, end1, end2, dtype)
    dev = pme_deviation(got, y1, end_got, end1, dtype)
    print("yardstick against itself:", repeat)
    print("recorded against the yardstick:", dev)
    for k in dev:
        if PME_REPEAT[dtype][k] == 0.0:
            assert dev[k] == 0.0, (k, dev, repeat)
        else:
            assert dev[k] <= 3 * PME_REPEAT[dtype][k], (k, dev, repeat)


# ---- 6. continuation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vv", "langevin"])
def test_chunked_recorded_runs_continue_one_history(pkg, kind):
    L = pkg.lib()
    one, end_one, _, _ = recorded(pkg, "edge257", np.float64, EVERY, [(0, 25)], kind, 0)
    two, end_two, _, s = recorded(pkg, "edge257", np.float64, EVERY, [(0, 12), (12, 13)], kind, 0)
    assert_same_history(two, one)
    assert end_two == end_one
    assert info_of(L, s) == [[3, 8, 8, 24], [6, 4, 4, 24], [5, 5, 5, 25], [10, 2, 2, 20]]
    ok(L, s, L.mhip_record_clear(s._ctx))
    assert info_of(L, s) == [[3, 8, 0, -1], [6, 4, 0, -1], [5, 5, 0, -1], [10, 2, 0, -1]]
    ok(L, s, run_call(L, s, kind, 25, 5, 0.002, 0, 25))      # the buffers are still there: steps 27 and 30
    assert [r[2:] for r in info_of(L, s)] == [[2, 30], [1, 30], [1, 30], [1, 30]]


# ---- 7. fusing survives --------------------------------------------------------------------------------------------------------------------------
def test_steps_between_records_keep_their_fused_form(pkg):
    _, _, st_want = yardstick(pkg, "packed", np.float32, EVERY, [(0, 25)])
    _, _, st_got, _ = recorded(pkg, "packed", np.float32, EVERY, [(0, 25)])
    n_record_steps = len({st for st in range(1, 26) if mask_at(EVERY, st)})
    assert n_record_steps == 12
    assert st_got["n_fused_steps"] == st_want["n_fused_steps"] and st_got["n_fused_steps"] >= max(1, 25 - 2 * n_record_steps), (st_got["n_fused_steps"], st_want["n_fused_steps"])
    assert st_got["n_force_calls"] <= st_want["n_force_calls"]      # (the yardstick's potential energies are force calls of its own)


# ---- 8. refusals and capacity ----------------------------------------------------------------------------------------------------------------------
def test_capacity_is_checked_before_anything_is_launched(pkg):
    L = pkg.lib()
    for kind in ("vv", "langevin"):
        s = fresh(pkg, "edge257", np.float64)
        ok(L, s, set_record(L, s, [3, 0, 0, 0], [2, 0, 0, 0]))
        ok(L, s, run_call(L, s, kind, 0, 6, 0.002, 1, 0))      # two records fit
        before = (info_of(L, s), read_channel(L, s, KE)[1].tobytes(), final_state(L, s))
        assert run_call(L, s, kind, 6, 9, 0.002, 1, 0) == ERR_CAPACITY      # three records due, none fits
        assert b"capacity" in L.mhip_last_error(s._ctx)
        assert run_call(L, s, kind, 6, 3, 0.002, 1, 0) == ERR_CAPACITY      # one due
        assert (info_of(L, s), read_channel(L, s, KE)[1].tobytes(), final_state(L, s)) == before
        ok(L, s, run_call(L, s, kind, 6, 2, 0.002, 1, 0))      # a run that records nothing is admitted by a full channel
        assert L.mhip_record_now(s._ctx, 8, 1) == ERR_CAPACITY
        ok(L, s, L.mhip_record_clear(s._ctx))
        ok(L, s, L.mhip_record_now(s._ctx, 8, 1))


def test_invalid_arguments(pkg):
    L = pkg.lib()
    s = fresh(pkg, "edge257", np.float64)
    assert set_record(L, s, [-1, 0, 0, 0], [1, 0, 0, 0]) == ERR_INVALID       # a negative interval
    assert set_record(L, s, [5, 0, 0, 0], [0, 0, 0, 0]) == ERR_INVALID        # on, without room
    assert set_record(L, s, [0, 0, 5, 0], [0, 0, -3, 0]) == ERR_INVALID
    assert L.mhip_set_record(s._ctx, None, None) == ERR_INVALID
    assert L.mhip_record_now(s._ctx, 0, 1) == ERR_INVALID                     # no recorder: no buffer
    ok(L, s, set_record(L, s, [5, 0, 0, 0], [4, 0, 0, 0]))
    assert L.mhip_record_now(s._ctx, 0, 1 << X) == ERR_INVALID                # a channel that is off
    assert L.mhip_record_now(s._ctx, 0, 16) == ERR_INVALID and L.mhip_record_now(s._ctx, 0, -1) == ERR_INVALID
    ok(L, s, L.mhip_record_now(s._ctx, 0, 1))
    steps, vals = np.zeros(4, np.int64), np.zeros(4)
    for c, first, n in [(KE, 0, 2), (KE, 1, 1), (KE, -1, 1), (KE, 0, -1), (X, 0, 1), (4, 0, 0), (-1, 0, 0)]:      # beyond the records held, or no such channel
        assert L.mhip_record_read(s._ctx, c, first, n, p(steps), p(vals), 0) == ERR_INVALID, (c, first, n)
    assert L.mhip_record_read(s._ctx, KE, 0, 1, p(steps), p(vals), 7) == ERR_INVALID
    ok(L, s, L.mhip_record_read(s._ctx, KE, 0, 1, None, p(vals), 0))          # steps_out may be null
    ok(L, s, L.mhip_record_read(s._ctx, KE, 1, 0, p(steps), p(vals), 0))      # an empty range at the end
    assert L.mhip_record_info(s._ctx, None) == ERR_INVALID
    assert info_of(L, s)[KE] == [5, 4, 1, 0]
    ok(L, s, set_record(L, s, [5, 0, 0, 0], [4, 0, 0, 0]))                    # setting always empties the history
    assert info_of(L, s)[KE] == [5, 4, 0, -1]


def test_loops_that_do_not_record_refuse_a_recorder(pkg):
    L = pkg.lib()
    s, twin = fresh(pkg, "edge257", np.float64), fresh(pkg, "edge257", np.float64)
    ok(L, s, set_record(L, s, [5, 0, 0, 0], [64, 0, 0, 0]))
    done, reason = C.c_int64(0), C.c_int32(0)
    log4, out8 = np.zeros((4, 4)), np.zeros(8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    calls = {
        "mhip_splitting_run": lambda c: L.mhip_splitting_run(c._ctx, 0, 2, 0.002, KB * 120.0, 2.0, b"BAOAB", 1, KEY, CTR1),
        "mhip_overdamped_run": lambda c: L.mhip_overdamped_run(c._ctx, 0, 2, 0.0001, KB * 120.0, 50.0, 1, KEY, CTR1),
        "mhip_minimize": lambda c: L.mhip_minimize(c._ctx, 0, 2, 0.01, 1000.0, 0.0, dp(log4), dp(out8)),
        "mhip_domain_run": lambda c: L.mhip_domain_run(c._ctx, 0, 2, 0.002, 0, None, 0, C.byref(done), C.byref(reason), None)}
    for what, call in calls.items():
        assert call(s) == ERR_UNSUPPORTED, what
        msg = L.mhip_last_error(s._ctx).decode()
        assert what in msg and "recorder" in msg, msg
    ok(L, s, set_record(L, s, [0] * 4, [0] * 4))
    for what, call in calls.items():      # admitted again: each answers what it answers on a context that never had a recorder
        a, b = call(s), call(twin)
        assert a == b and (a == OK or "recorder" not in L.mhip_last_error(s._ctx).decode()), (what, a, b)
    assert final_state(L, s) == final_state(L, twin)


def test_recorder_against_ghosts_and_plans(pkg):
    """the walk of tests/admit_walk.py: with the recorder on every ghosted / domain entry point refuses and the run goes on; with a plan there first mhip_set_record
    refuses, switching off is allowed, and the recorder is taken once the plan is gone"""
    L = pkg.lib()
    case = case_of("edge257")[0]
    on = lambda s: set_record(L, s, [2, 0, 2, 0], [64, 0, 64, 0])
    off = lambda s: set_record(L, s, [0] * 4, [0] * 4)
    admit_walk.walk(pkg, case, on, off)
    s = fresh(pkg, "edge257", np.float64)
    ok(L, s, L.mhip_set_atom_counts(s._ctx, 200, 57))      # a context with ghosts
    assert on(s) == ERR_UNSUPPORTED and "ghosts" in L.mhip_last_error(s._ctx).decode()
    ok(L, s, off(s))
    s = fresh(pkg, "edge257", np.float64)
    ok(L, s, on(s))
    assert L.mhip_set_atom_counts(s._ctx, 200, 57) == ERR_UNSUPPORTED and "recorder" in L.mhip_last_error(s._ctx).decode()


@pytest.mark.parametrize("name,dtype", [("edge257", np.float64), ("packed", np.float32)], ids=["edge257-float64", "packed-float32"])
def test_a_recorder_switched_off_leaves_no_trace(pkg, name, dtype):
    L = pkg.lib()
    _, dt, cm = case_of(name)

    def run(with_recorder):
        s = fresh(pkg, name, dtype)
        ok(L, s, L.mhip_set_profiling(s._ctx, 1))
        if with_recorder:
            ok(L, s, set_record(L, s, [2, 4, 2, 2], [8, 8, 8, 8]))
            ok(L, s, L.mhip_record_now(s._ctx, 0, 15))
            ok(L, s, set_record(L, s, [0] * 4, [0] * 4))
            assert info_of(L, s) == [[0, 0, 0, -1]] * 4
        else:
            host_reads(L, s, 0, 15)      # the same reads through the entry points (the first of them searches the lists, as the record's does)
        calls0 = s.stats()["prof_calls"]
        ok(L, s, L.mhip_vv_run(s._ctx, 0, 20, dt, cm))
        st = s.stats()
        return final_state(L, s), [a - b for a, b in zip(st["prof_calls"], calls0)], st["n_fused_steps"]
    a, b = run(True), run(False)
    assert a[0] == b[0], "the state differs from that of a context that never had a recorder"
    assert a[1] == b[1] and a[2] == b[2], (a[1:], b[1:])


# ---- 9. the Python mirror --------------------------------------------------------------------------------------------------------------------------
def py_system(pkg, dtype=np.float64):
    return case_of("edge257")[0].system(pkg, dtype)


def with_loggers(pkg, s):
    s.loggers = {"temp": pkg.TemperatureLogger(5), "total": pkg.TotalEnergyLogger(10), "coords": pkg.CoordinatesLogger(10), "ke": pkg.KineticEnergyLogger(5)}
    return s


@pytest.mark.parametrize("run_loggers,lengths", [(True, (7, 4, 4)), ("skipstart", (6, 3, 3)), (False, (0, 0, 0))])
def test_simulate_fills_the_loggers(pkg, run_loggers, lengths):
    from molly_jl_amd import api
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=0)
    s = with_loggers(pkg, py_system(pkg))
    pkg.simulate(s, sim, 30, run_loggers=run_loggers)
    temp, total, coords, ke = (s.loggers[k] for k in ("temp", "total", "coords", "ke"))
    assert (len(temp.history), len(total.history), len(coords.history)) == lengths
    # the host loop: 5-step simulate calls with the energies and coordinates read in between
    h = py_system(pkg)
    log = {0: (pkg.kinetic_energy(h), pkg.potential_energy(h, 0), h.coords.copy())}
    for k in range(6):
        pkg.simulate(h, sim, 5, init_step=5 * k)
        log[5 * k + 5] = (pkg.kinetic_energy(h), pkg.potential_energy(h, 5 * k + 5), h.coords.copy())
    assert np.array_equal(s.coords, h.coords) and np.array_equal(s.velocities, h.velocities)
    if run_loggers is False:
        return
    assert temp.steps == ke.steps == [st for st in range(0, 31, 5) if st or run_loggers is True] and total.steps == coords.steps == [st for st in range(0, 31, 10) if st or run_loggers is True]
    assert ke.history == [log[st][0] for st in ke.steps]
    assert total.history == [log[st][0] + log[st][1] for st in total.steps]
    assert all(np.array_equal(f, log[st][2]) and f.dtype == s.dtype for f, st in zip(coords.history, coords.steps))
    assert temp.history == [2 * k / (api._df(s) * pkg.BOLTZMANN) for k in ke.history]      # exactly
    assert pkg.values(temp) is temp.history
    # the recorder is switched off behind the call: the context runs a simulator that does not record
    pkg.simulate(s, pkg.LangevinSplitting(dt=0.002, temperature=120.0, friction=1.0, splitting="BAOAB"), 2, run_loggers=False, rng=3)


@pytest.mark.parametrize("which", ["langevin", "barostat7", "barostat10"])
def test_simulate_with_langevin_and_with_a_barostat(pkg, which):
    """history lengths and step numbers; barostat10: the barostat applies on record steps, whose coordinates and energies are then taken behind its move"""
    s = with_loggers(pkg, py_system(pkg))
    if which == "langevin":
        sim = pkg.Langevin(dt=0.002, temperature=120.0, friction=1.0)
    else:
        sim = pkg.VelocityVerlet(dt=0.002, coupling=pkg.MonteCarloBarostat(1.0, 120.0, s.boundary, n_steps=int(which[8:])))
    pkg.simulate(s, sim, 30, rng=11)
    temp, total, coords = (s.loggers[k] for k in ("temp", "total", "coords"))
    assert temp.steps == list(range(0, 31, 5)) and total.steps == coords.steps == [0, 10, 20, 30]
    assert (len(temp.history), len(total.history), len(coords.history)) == (7, 4, 4)
    assert all(np.isfinite(v) for v in temp.history + total.history) and all(np.isfinite(f).all() for f in coords.history)


def test_simulators_that_do_not_record_refuse_loggers_on_the_device(pkg):
    s = with_loggers(pkg, py_system(pkg))
    with pytest.raises(pkg.MollyHipError) as e:
        pkg.simulate(s, pkg.LangevinSplitting(dt=0.002, temperature=120.0, friction=1.0, splitting="BAOAB"), 5)
    assert e.value.code == ERR_UNSUPPORTED
    assert all(lg.history == [] for lg in s.loggers.values())
