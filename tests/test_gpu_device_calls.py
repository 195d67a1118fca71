"""The C ABI's device-pointer call forms (mem_kind = MHIP_MEM_DEVICE on the caller's stream), as the Julia override drives them
(julia/ext/MollyHIPExt.jl): mhip_set_stream to the task's stream, set_state(dev x) + mhip_forces(step_n, accumulate = 1, dev fs_mat, host virial9),
the remove_CM_motion! round trip set_state(x, v) → mhip_remove_cm → get_state(NULL, v), and run_chunks!'s set_state → run → get_state.  A torch
device tensor stands in for the ROCArray (same packed xyz layout, a data_ptr and a stream).  Every test works on a NON-default torch stream, never
synchronises the device between torch writes and engine calls, and keeps the stream and every tensor alive until the context is destroyed.

The host-memory form stages through the engine's buffers and synchronises; the device form launches straight into (or reads straight from) the
caller's memory and rests on stream order alone.  So each check here compares the device form with the oracle, and — where the pair path is
deterministic (no float atomics) — bit for bit with the host form on a twin context."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import golden6mrr as G
from tests import systems as S
from tests.test_gpu_stochastic import draws

pytestmark = pytest.mark.gpu

HOST, DEV = 0, 1
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
KB = 8.314462618e-3


def _p(a):
    """a device tensor's or a numpy array's address, NULL for None"""
    if a is None:
        return None
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def _dev(a, dtype):
    """a (n, 3) device tensor of `a` in the working precision, made on the current stream"""
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


class Ctx:
    """A System's engine context driven through the raw ABI: set up by the System (case.system, s.engine()), then only mhip_* calls."""

    def __init__(self, pkg, case, dtype, stream=None):
        self.s = case.system(pkg, dtype)
        self.L, self.ctx = pkg.lib(), self.s.engine()
        if stream is not None:
            self.ok(self.L.mhip_set_stream(self.ctx, C.c_void_p(stream.cuda_stream)))

    def ok(self, rc):
        self.s._check(rc)

    def __getattr__(self, name):         # ctx.set_state(...) → mhip_set_state(ctx, ...), status checked
        fn = getattr(self.L, "mhip_" + name)
        return lambda *a: self.ok(fn(self.ctx, *a))

    def stats(self):
        return self.s.stats()

    def close(self):
        self.s.close()


def _pattern(n, dtype, scale):
    """a non-zero force pattern, distinct in every element, of about the forces' magnitude"""
    k = np.arange(3 * n, dtype=np.float64)
    return (scale * (2.0 * ((k * 0.6180339887498949 + 0.1234) % 1.0) - 1.0)).astype(dtype).reshape(n, 3)


V0 = np.array([1.5, -2.25, 0.75, -2.25, 3.0, 0.5, 0.75, 0.5, -1.25])     # exact binary fractions: virial9 − V0 is exact where W is


def _case_a(kind, dtype):
    if kind == "lj":
        return S.lj_fluid(12, dtype=dtype)
    if kind == "rf":
        return S.charged_fluid(10, dict(kind="rf", rc=1.0, weight_special=0.8333333333333334), dtype=dtype, stable=True)
    if dtype == np.float64:                                    # 15 954 atoms, not a multiple of 256; pair + bonded + PME into one device buffer
        return G.case("ewald", np.float64, bonded=True, approx_erfc=False, pme=True)
    return G.case("rf", dtype, bonded=False)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["lj", "rf", "6mrr"])
def test_accumulate_into_device_buffer_with_virial(pkg, slack, kind, dtype):
    """engine_forces! (MollyHIPExt.jl:123-133): set_state(dev x, NULL) → mhip_forces(step_n, accumulate = 1, dev fs_mat, host virial9) into buffers
    that already hold something.  k_export_forces adds through orig[cur] into the caller's rows: out == P + f bit for bit (f from the host form on a twin
    context), out − P against the oracle, virial9 − V0 against the oracle's pair virial.  accumulate = 0 into a NaN-filled buffer writes every owned
    row exactly once.  6mrr fp64: the specific and general forces follow into the same device buffer, the total against OpenMM."""
    case = _case_a(kind, dtype)
    n, step_n = case.n, 0
    if dtype == np.float64:
        o = case.oracle(np.float64)
        nl = o.neighbors("cell", nthreads=8)
    else:
        tol, o, nl = S.fp32_force_tolerance(case)
    f_ref = o.forces(nl, nthreads=8)
    w_ref = o.virial(nl)
    P = _pattern(n, dtype, float(np.sqrt((f_ref ** 2).mean())))

    twin = Ctx(pkg, case, dtype)                               # the host-memory form of the same call sequence
    try:
        f_host = np.zeros((n, 3), dtype); w_host = np.zeros(9); f_host2 = np.zeros((n, 3), dtype)
        x_host = np.ascontiguousarray(case.coords, dtype=dtype)
        twin.set_state(_p(x_host), None, HOST)
        twin.forces(step_n, 1, _p(f_host), _p(w_host), HOST)
        if case.pme is not None:
            f_rest = np.zeros((n, 3), dtype)
            twin.specific_forces(1, _p(f_rest), HOST)
            twin.general_forces(1, _p(f_rest), HOST)
        twin.forces(step_n, 0, _p(f_host2), None, HOST)
    finally:
        twin.close()

    st = torch.cuda.Stream()
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            x = _dev(case.coords, dtype)
            f = torch.tensor(P, device="cuda")
            vir = V0.copy()
            e.set_state(_p(x), None, DEV)
            e.forces(step_n, 1, _p(f), _p(vir), DEV)
            out_pair = f.clone()                               # read on the stream, behind the export
            if case.pme is not None:
                e.specific_forces(1, _p(f), DEV)
                e.general_forces(1, _p(f), DEV)
            f_nan = torch.full((n, 3), float("nan"), dtype=TORCH[np.dtype(dtype)], device="cuda")
            e.forces(step_n, 0, _p(f_nan), None, DEV)
            out_nan = f_nan.clone()
        st.synchronize()
        out, out_total, out0 = out_pair.cpu().numpy(), f.cpu().numpy(), out_nan.cpu().numpy()
    finally:
        e.close()

    assert np.array_equal(out, P + f_host), f"device accumulate differs from P + host form in {int((out != P + f_host).sum())} elements"
    assert np.array_equal(vir, V0 + w_host)
    # (the second pass at the same coordinates is compared with the twin's second pass, not with the first: the first plain pass after a search of a
    # dual list walks the outer list and prunes it, later passes walk the inner list, and in fp32 the two orders of the sums differ in the last bits)
    assert not np.isnan(out0).any() and np.array_equal(out0, f_host2)

    err = np.linalg.norm(out.astype(np.float64) - P.astype(np.float64) - f_ref, axis=1)
    w = (vir - V0).reshape(3, 3)
    wscale = np.abs(w_ref).max()
    if dtype == np.float64:
        slack("pair forces accumulated into a device buffer vs the fp64 oracle, kJ/mol/nm (test/protein.jl:267)", err.max(), 1e-7)
    else:
        S.fp32_check(err, tol, "pair forces accumulated into a device buffer vs the fp64 oracle")
    rel = (1e-9 if dtype == np.float64 else 3e-4) if kind == "6mrr" else (1e-10 if dtype == np.float64 else 2e-4)
    slack("pair virial of the device-form call vs the oracle, / max|W|", np.abs(w - w_ref).max() / wscale, rel)
    if case.pme is not None:                                   # float atomics in the bonded and mesh paths: the oracle bar only
        d = G.data()
        err_all = np.linalg.norm(out_total - P - d["openmm_forces_all_pme_exact"], axis=1)
        slack("pair + specific + general forces in one device buffer vs OpenMM all_pme_exact, kJ/mol/nm", err_all.max(), 1e-6)


def test_calls_are_ordered_on_the_callers_stream(pkg, slack):
    """mhip_set_stream puts the engine's work on the caller's stream; with device pointers nothing else orders the engine behind the caller's writes.
    Torch work holds the stream for milliseconds, behind it the coordinates are overwritten in place (x1 = x0 + 0.01 nm per atom); set_state + forces
    queued at once, and a torch read of the force buffer behind them, must see the forces at x1.  Then the other direction: coordinates rewritten behind
    more queued work, set_state, get_state into a device tensor and at once a torch read of it, which must hold the new coordinates."""
    dtype = np.float64
    case = S.lj_fluid(12, dtype=dtype)
    n, L = case.n, float(case.box[0])
    rng = np.random.default_rng(11)

    def moved(x):
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        y = x + 0.01 * u
        y -= np.floor(y / L) * L
        return np.where(y >= L, 0.0, y)
    x0 = case.coords
    x1 = moved(x0); x2 = moved(x1)
    o1 = case.oracle(np.float64, coords=x1)
    f1_ref = o1.forces(o1.neighbors("cell", nthreads=8), nthreads=8)
    o0 = case.oracle(np.float64)
    f0_ref = o0.forces(o0.neighbors("cell", nthreads=8), nthreads=8)
    assert np.linalg.norm(f1_ref - f0_ref, axis=1).max() > 1e3 * 1e-7      # the forces at x0 would fail the bar by far

    st = torch.cuda.Stream()
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            x = _dev(x0, dtype); x1_d = _dev(x1, dtype); x2_d = _dev(x2, dtype)
            f = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            xo = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            a = torch.randn((8192, 8192), dtype=torch.float32, device="cuda")
            c = torch.empty_like(a)
            e.set_state(_p(x), None, DEV)
            e.forces(0, 0, _p(f), None, DEV)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(st)
            for _ in range(4):
                torch.mm(a, a, out=c)                          # hold the stream
            x.copy_(x1_d)
            ev[1].record(st)
            e.set_state(_p(x), None, DEV)
            e.forces(1, 0, _p(f), None, DEV)
            f_read = f.clone()
            ev[2].record(st)
            for _ in range(4):
                torch.mm(a, a, out=c)
            x.copy_(x2_d)
            ev[3].record(st)
            e.set_state(_p(x), None, DEV)
            xo.fill_(float("nan"))
            e.get_state(_p(xo), None, DEV)
            x_read = xo.clone()
        st.synchronize()
        window_ms = (ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]))
        f_got, x_got = f_read.cpu().numpy(), x_read.cpu().numpy()
    finally:
        e.close()
    print(f"[ordering] queued work ahead of the overwrites: {window_ms[0]:.1f} ms, {window_ms[1]:.1f} ms")
    slack("forces behind an in-place coordinate overwrite on the caller's stream vs the oracle at x1, kJ/mol/nm", np.linalg.norm(f_got - f1_ref, axis=1).max(), 1e-7)
    assert np.array_equal(x_got, x2), "get_state into device memory: the stream's next read did not see the engine's coordinates"


def _stock_vv(pkg, case, mem, n_steps, dt, st, vir_every=10):
    """simulate!(sys, ::VelocityVerlet) of the reference (simulators.jl:547-668) with the overridden forces! and remove_CM_motion! (MollyHIPExt.jl):
    the integrator in torch on the device, the engine seeing only set_state + forces(step_n) and the CM round trip.  mem = HOST: the same loop through
    the host-memory form (copies on the stream's side of the boundary, same torch arithmetic)."""
    T = np.float64
    e = Ctx(pkg, case, T, st)
    n = case.n
    try:
        with torch.cuda.stream(st):
            box = torch.tensor(case.box, dtype=torch.float64, device="cuda")
            x = _dev(case.coords, T); v = _dev(case.velocities, T)
            m = torch.tensor(case.mass, dtype=torch.float64, device="cuda")[:, None]
            keep = []

            def set_state(xx, vv):
                if mem == DEV:
                    e.set_state(_p(xx), _p(vv), DEV)
                else:
                    hx = xx.cpu().numpy(); hv = None if vv is None else vv.cpu().numpy()
                    keep.append((hx, hv))
                    e.set_state(_p(hx), _p(hv), HOST)

            def forces(step_n, vir):
                set_state(x, None)
                if mem == DEV:
                    f = torch.zeros((n, 3), dtype=torch.float64, device="cuda")        # buffers.fs_mat, zeroed by the caller (force.jl:1216)
                    e.forces(step_n, 1, _p(f), _p(vir), DEV)
                    return f
                fh = np.zeros((n, 3))
                e.forces(step_n, 1, _p(fh), _p(vir), HOST)
                return torch.from_numpy(fh).to("cuda")

            def remove_cm():
                set_state(x, v)
                e.remove_cm()
                if mem == DEV:
                    e.get_state(None, _p(v), DEV)
                else:
                    hv = np.empty((n, 3)); e.get_state(None, _p(hv), HOST); v.copy_(torch.from_numpy(hv))

            x.sub_(torch.floor(x / box) * box)
            remove_cm()
            a = forces(0, None) / m
            virials = []
            for step_n in range(1, n_steps + 1):
                v.add_(a * dt / 2)
                x.add_(v * dt)
                x.sub_(torch.floor(x / box) * box)
                vir = np.zeros(9) if step_n % vir_every == 0 else None
                a = forces(step_n, vir) / m
                v.add_(a * dt / 2)
                remove_cm()
                if vir is not None:
                    virials.append((x.clone(), vir))
        st.synchronize()
        return x.cpu().numpy(), v.cpu().numpy(), [(xx.cpu().numpy(), w.reshape(3, 3)) for xx, w in virials], e.stats()
    finally:
        e.close()


def test_stock_velocity_verlet_over_device_forces(pkg, slack):
    """The caller owns the integrator over 50 steps (the reference's generic loop calling the overridden forces! at every step, virial on every 10th),
    the engine sees set_state + forces(step_n) only — the displacement check of lists_after_set_state fed from device memory, across the rebuild steps
    10 … 40.  Against the oracle's velocity Verlet at the C client's bars; the list decisions and the trajectory bit-identical to the host-memory form."""
    case = S.lj_fluid(16, dtype=np.float64)
    n_steps, dt = 50, 0.002
    st = torch.cuda.Stream()
    x, v, virials, stats = _stock_vv(pkg, case, DEV, n_steps, dt, st)
    xh, vh, _, stats_h = _stock_vv(pkg, case, HOST, n_steps, dt, st)
    o = case.oracle(np.float64)
    o.vv_run(n_steps, dt, remove_cm_every=1, nthreads=8)
    d = x - o.coords
    d -= np.round(d / case.box) * case.box
    slack("stock VV loop over device-form forces: coordinates vs the oracle after 50 steps, nm", np.abs(d).max(), 1e-9)
    slack("stock VV loop over device-form forces: velocities vs the oracle after 50 steps, nm/ps", np.abs(v - o.vel).max(), 1e-8)
    assert len(virials) == n_steps // 10
    worst = 0.0
    for xk, w in virials:
        ok = case.oracle(np.float64, coords=xk)
        w_ref = ok.virial(ok.neighbors("cell", nthreads=8))
        worst = max(worst, np.abs(w - w_ref).max() / np.abs(w_ref).max())
    slack("virial requested inside the stock loop vs the oracle at the step's coordinates, / max|W|", worst, 1e-10)
    keys = ("n_outer_builds", "n_filter_passes", "n_rebuilds")
    assert {k: stats[k] for k in keys} == {k: stats_h[k] for k in keys}
    assert stats["n_rebuilds"] >= 1
    assert np.array_equal(x, xh) and np.array_equal(v, vh)


def _chunked(pkg, case, dtype, st, run):
    """run_chunks! (MollyHIPExt.jl:215-245): set_state(dev x, dev v) → run(first, n) → get_state(dev x, dev v) → set_state(the same tensors) → …
    25 steps cut at 7 and 14 (rebuild steps 10 and 20 inside chunks)"""
    e = Ctx(pkg, case, dtype, st)
    try:
        with torch.cuda.stream(st):
            x = _dev(case.coords, dtype); v = _dev(case.velocities, dtype)
            for first, n in ((0, 7), (7, 7), (14, 11)):
                e.set_state(_p(x), _p(v), DEV)
                run(e, first, n)
                e.get_state(_p(x), _p(v), DEV)
        st.synchronize()
        return x.cpu().numpy(), v.cpu().numpy()
    finally:
        e.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunked_vv_through_device_pointers_is_exact(pkg, dtype):
    """the case of test_chunked_continuation_is_exact_without_cm_removal, chunks handed over in device memory: bit-identical to one uncut run"""
    case = S.lj_fluid(10, dtype=dtype)
    sim = pkg.VelocityVerlet(dt=0.002, remove_CM_motion=0)
    a = case.system(pkg, dtype)
    pkg.simulate(a, sim, 25)
    x, v = _chunked(pkg, case, dtype, torch.cuda.Stream(), lambda e, first, n: e.vv_run(first, n, 0.002, 0))
    assert np.array_equal(x, a.coords) and np.array_equal(v, a.velocities)
    a.close()


def test_chunked_langevin_through_device_pointers_is_exact(pkg):
    """mhip_langevin_run in chunks with the shim's counter rule ctr1 + (first − init_step) (MollyHIPExt.jl:284; include/mollyhip.h: step first + s uses
    ctr1 + s − 1): bit-identical to the uncut run in fp64"""
    dtype = np.float64
    case = S.lj_fluid(10, dtype=dtype)
    sim = pkg.Langevin(dt=0.002, temperature=85.0, friction=1.0, remove_CM_motion=0)
    a = case.system(pkg, dtype)
    pkg.simulate(a, sim, 25, rng=21)
    key, ctr1 = draws(21, 2)                                   # simulate's order: key, then ctr1 (simulators.jl:1149-1150)
    kT = KB * 85.0

    def run(e, first, n):
        e.langevin_run(first, n, 0.002, kT, 1.0, 0, key, (ctr1 + first) % 2 ** 64)
    x, v = _chunked(pkg, case, dtype, torch.cuda.Stream(), run)
    assert np.array_equal(x, a.coords) and np.array_equal(v, a.velocities)
    a.close()
