"""The host side of the loggers (molly.jl_amd/api.py): the logger classes' constructors, what simulate() asks of the engine's recorder — one interval per
channel, the gcd of the loggers that need it, and the capacity of the run — and how it deals the records out again, the run_loggers values of
loggers.jl:47-55.  No GPU: simulate() runs against a stand-in library that keeps a recorder's history on the host (every value is made of its step number)."""
import ctypes as C

import numpy as np
import pytest


LOGGERS = ("TemperatureLogger", "KineticEnergyLogger", "PotentialEnergyLogger", "TotalEnergyLogger", "CoordinatesLogger", "VelocitiesLogger")


def test_logger_constructors(pkg):
    for name in LOGGERS:
        cls = getattr(pkg, name)
        lg = cls(10)
        assert lg.n_steps == 10 and lg.history == [] and pkg.values(lg) is lg.history
        for bad in (0, -1, 2.5):
            with pytest.raises(ValueError):
                cls(bad)
    s = pkg.System(coords=np.zeros((4, 3)), boundary=pkg.CubicBoundary(2.0), loggers={"temp": pkg.TemperatureLogger(10)})
    assert list(s.loggers) == ["temp"]
    assert pkg.System(coords=np.zeros((4, 3)), boundary=pkg.CubicBoundary(2.0)).loggers == {}
    with pytest.raises(pkg.MollyHipError) as e:
        pkg.System(coords=np.zeros((4, 3)), boundary=pkg.CubicBoundary(2.0), loggers={"forces": object()})      # no logger the engine does not record
    assert e.value.code == -6


def test_record_plan_gcd_and_capacity(pkg):
    from molly_jl_amd import api
    T, K, P, E, X, V = (getattr(pkg, n) for n in LOGGERS)
    plan = api._record_plan
    # the reference's first documented example: temperature and coordinates every 10 steps
    assert plan([T(10), X(10)], 0, 1000) == ([10, 0, 10, 0], [101, 0, 101, 0], 0b0101)
    # the gcd per channel: KE is needed by T(5), E(10) and K(4); PE by E(10) and P(15)
    assert plan([T(5), E(10), K(4), P(15), X(10), V(7)], 0, 30) == ([1, 5, 10, 7], [31, 7, 4, 5], 0b1111)
    # 'skipstart': no record of step 0, but one of an init_step that is not 0 (loggers.jl:50)
    assert plan([T(5), E(10), X(10)], 0, 30, "skipstart") == ([5, 10, 10, 0], [6, 3, 3, 0], 0)
    assert plan([T(5), E(10), X(10)], 10, 30, "skipstart") == ([5, 10, 10, 0], [7, 4, 4, 0], 0b0111)
    # an init_step at which only some loggers are due; a run shorter than an interval keeps room for one record
    assert plan([T(5), X(10)], 5, 4) == ([5, 0, 10, 0], [1, 0, 1, 0], 0b0001)
    assert plan([T(5), X(10)], 12, 13) == ([5, 0, 10, 0], [3, 0, 1, 0], 0)
    assert plan([T(5)], 0, 30, False) == ([0, 0, 0, 0], [0, 0, 0, 0], 0)
    for bad in ("start", None, 1.5, "skip"):
        with pytest.raises(ValueError):
            plan([T(5)], 0, 30, bad)


class StandIn:
    """libmollyhip's entry points as simulate() uses them, with the recorder's history kept here: KE of step s is s, PE is (s, 2s, 3s), a frame is filled with s"""

    def __init__(self, n_atoms):
        self.n, self.calls, self.every, self.cap, self.hist = n_atoms, [], [0] * 4, [0] * 4, [[] for _ in range(4)]

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            f = getattr(type(self), "do_" + name[5:], None)      # (every other entry point: status 0)
            return f(self, *args) if f else 0
        return call

    def do_create(self, ctx_ref, cfg):
        ctx_ref._obj.value = 1
        return 0

    def do_set_record(self, ctx, every, cap):
        self.every, self.cap, self.hist = list(every._obj), list(cap._obj), [[] for _ in range(4)]
        return 0

    def record(self, step, mask):
        for c in range(4):
            if (mask >> c) & 1:
                assert self.every[c] > 0 and len(self.hist[c]) < self.cap[c], (c, step, self.every, self.cap)
                self.hist[c].append(step)

    def do_record_now(self, ctx, step, mask):
        self.record(step, mask)
        return 0

    def run(self, ctx, first, n, *rest):
        for s in range(first + 1, first + n + 1):
            self.record(s, sum(1 << c for c in range(4) if self.every[c] and s % self.every[c] == 0))
        return 0

    do_vv_run = do_langevin_run = run

    def do_record_info(self, ctx, out):
        for c in range(4):
            out._obj[4 * c: 4 * c + 4] = [self.every[c], self.cap[c], len(self.hist[c]), self.hist[c][-1] if self.hist[c] else -1]
        return 0

    def do_record_read(self, ctx, c, first, n, steps, values, mem_kind):
        s = np.array(self.hist[c][first:first + n], np.int64)
        C.memmove(steps, s.ctypes.data, s.nbytes)
        w = (1, 3, 3 * self.n, 3 * self.n)[c]
        v = np.repeat(s.astype(np.float64), w).reshape(n, w)
        if c == 1:
            v *= [1, 2, 3]
        v = v.astype(np.float64 if c < 2 else np.float32)
        C.memmove(values, v.ctypes.data, v.nbytes)
        return 0


@pytest.fixture
def stand_in(pkg, monkeypatch):
    from molly_jl_amd import _lib
    made = []

    def lib():
        if not made:
            made.append(StandIn(4))
        return made[0]
    monkeypatch.setattr(_lib, "lib", lib)
    yield lib
    while SYSTEMS:
        SYSTEMS.pop()._ctx = None      # the stand-in's handle is not the library's to destroy


SYSTEMS = []


def make_system(pkg, **loggers):
    SYSTEMS.append(_make_system(pkg, **loggers))
    return SYSTEMS[-1]


def _make_system(pkg, **loggers):
    return pkg.System(coords=np.random.default_rng(0).uniform(0, 2, (4, 3)), boundary=pkg.CubicBoundary(2.0), pairwise_inters=(pkg.LennardJones(),), dtype=np.float32, loggers=loggers)


@pytest.mark.parametrize("run_loggers,lengths", [(True, (7, 4, 4)), ("skipstart", (6, 3, 3)), (False, (0, 0, 0))])
def test_simulate_deals_the_records_to_the_loggers(pkg, stand_in, run_loggers, lengths):
    from molly_jl_amd import api
    s = make_system(pkg, temp=pkg.TemperatureLogger(5), total=pkg.TotalEnergyLogger(10), coords=pkg.CoordinatesLogger(10))
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.001), 30, run_loggers=run_loggers)
    L = stand_in()
    temp, total, coords = (s.loggers[k] for k in ("temp", "total", "coords"))
    assert (len(temp.history), len(total.history), len(coords.history)) == lengths
    first = 0 if run_loggers is True else 1
    assert temp.steps == [5 * k for k in range(first, 7)][:lengths[0]] and total.steps == coords.steps == [10 * k for k in range(first, 4)][:lengths[1]]
    if run_loggers is False:
        assert "mhip_set_record" not in L.calls and "mhip_record_read" not in L.calls      # exactly the calls of a System without loggers
        return
    assert temp.history == [2 * float(st) / (api._df(s) * pkg.BOLTZMANN) for st in temp.steps]
    assert total.history == [float(st) + (0.0 + st + 2 * st + 3 * st) for st in total.steps]
    assert all(f.shape == (4, 3) and f.dtype == np.float32 and (f == st).all() for f, st in zip(coords.history, coords.steps))
    assert L.calls.count("mhip_set_record") == 2 and L.every == [0, 0, 0, 0]               # set for the call, switched off behind it
    assert L.calls.count("mhip_record_now") == (1 if run_loggers is True else 0)
    assert L.calls.count("mhip_record_read") == 3 and L.calls.count("mhip_vv_run") == 1     # read once at the end; the run is not cut


def test_simulate_continues_histories_and_cuts_only_for_the_barostat(pkg, stand_in):
    s = make_system(pkg, ke=pkg.KineticEnergyLogger(3), vel=pkg.VelocitiesLogger(10))
    pkg.simulate(s, pkg.Langevin(dt=0.001, temperature=100.0, friction=1.0), 12, rng=1)
    pkg.simulate(s, pkg.Langevin(dt=0.001, temperature=100.0, friction=1.0), 13, init_step=12, rng=1)      # 12 is a multiple of 3: recorded again, as the reference does
    assert s.loggers["ke"].steps == [0, 3, 6, 9, 12, 12, 15, 18, 21, 24] and s.loggers["vel"].steps == [0, 10, 20]
    assert stand_in().calls.count("mhip_langevin_run") == 2


def test_simulators_that_do_not_record_refuse_loggers(pkg, stand_in):
    s = make_system(pkg, temp=pkg.TemperatureLogger(5))
    for sim in (pkg.LangevinSplitting(dt=0.001, temperature=100.0, friction=1.0, splitting="BAOAB"), pkg.OverdampedLangevin(dt=0.001, temperature=100.0, friction=1.0),
                pkg.SteepestDescentMinimizer()):
        with pytest.raises(pkg.MollyHipError) as e:
            pkg.simulate(s, sim, 10)
        assert e.value.code == -6 and "loggers" in str(e.value)
    assert "mhip_splitting_run" not in stand_in().calls
    pkg.simulate(s, pkg.LangevinSplitting(dt=0.001, temperature=100.0, friction=1.0, splitting="BAOAB"), 10, run_loggers=False)      # without them: as before
    assert "mhip_splitting_run" in stand_in().calls and s.loggers["temp"].history == []
    with pytest.raises(ValueError):
        pkg.simulate(s, pkg.VelocityVerlet(dt=0.001), 10, run_loggers="always")
