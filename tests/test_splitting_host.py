"""LangevinSplitting and OverdampedLangevin without a GPU: (a) the numpy restatement (tests/splitting_ref.py) is pinned to the oracle's own integrators where a
splitting IS one of them — "BAB" is velocity Verlet, "BAOA" with friction = γ·m the Langevin-middle scheme; (b) the host-only plan (molly.jl_amd/csrc/splitting.h)
against the reference's regex-and-loop rule for every string over {A, B, O} up to length 6, and the inputs it rejects; (c) the C ABI carries both entry points."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import splitting_ref as R
from tests import systems as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molly.jl_amd", "csrc")
KB = 8.314462618e-3
BAR = 1e-12      # not a tuned number: anything above round-off means the restatement is wrong (measured 2.2e-16 nm / 8.7e-16 nm/ps and 2.2e-16 / 4.4e-16)


@pytest.fixture(scope="module")
def fluid():
    return S.lj_fluid(6, dtype=np.float64)


@pytest.mark.parametrize("remove_cm", [1, 0])
def test_bab_restatement_is_the_oracles_velocity_verlet(fluid, remove_cm):
    o = fluid.oracle(np.float64); o.vv_run(20, 0.002, remove_cm_every=remove_cm)
    r = fluid.oracle(np.float64)
    n_force = R.splitting_run(r, 20, 0.002, 0.0, 0.0, "BAB", remove_cm_every=remove_cm)
    dx, dv = np.abs(r.coords - o.coords).max(), np.abs(r.vel - o.vel).max()
    print("BAB against vv_run: max |dx|", dx, "max |dv|", dv)
    assert n_force == 20 and dx < BAR and dv < BAR


def test_baoa_restatement_is_the_oracles_langevin(fluid):
    gamma, key, ctr1 = 2.0, 0x9E3779B97F4A7C15, 2 ** 64 - 5      # (the counter wraps inside the run)
    o = fluid.oracle(np.float64); o.langevin_run(20, 0.002, KB * 85.0, gamma, key=key, ctr1=ctr1, remove_cm_every=1)
    r = fluid.oracle(np.float64)
    R.splitting_run(r, 20, 0.002, KB * 85.0, gamma * float(fluid.mass[0]), "BAOA", key=key, ctr1=ctr1, remove_cm_every=1)
    dx, dv = np.abs(r.coords - o.coords).max(), np.abs(r.vel - o.vel).max()
    print("BAOA against langevin_run: max |dx|", dx, "max |dv|", dv)
    assert dx < BAR and dv < BAR


def test_restatement_continues_in_chunks_and_leaves_massless_atoms_to_the_drift():
    case = S.lj_fluid(5, dtype=np.float64)
    case.mass = case.mass.copy(); case.mass[3] = 0.0
    a = case.oracle(np.float64); R.splitting_run(a, 12, 0.002, KB * 85.0, 80.0, "OBABO", key=7, ctr1=100)
    b = case.oracle(np.float64); R.splitting_run(b, 5, 0.002, KB * 85.0, 80.0, "OBABO", key=7, ctr1=100)
    R.splitting_run(b, 7, 0.002, KB * 85.0, 80.0, "OBABO", key=7, ctr1=100 + 5 * 2, first_step=5)
    # (a chunk starts with the forces of the coordinates held, recomputed on a fresh list: the same numbers up to the summation order)
    assert np.abs(a.coords - b.coords).max() < 1e-11 and np.abs(a.vel - b.vel).max() < 1e-11
    c = case.oracle(np.float64); v0 = c.vel[3].copy(); c.remove_cm(); v3 = c.vel[3].copy()
    c = case.oracle(np.float64); R.splitting_run(c, 1, 0.002, KB * 85.0, 80.0, "BOAB", key=7, ctr1=100, remove_cm_every=0)
    assert np.array_equal(c.vel[3], v0) and not np.array_equal(v0, v3)      # neither kicked nor thermalised
    x3 = case.coords[3] + v0 * 0.002
    assert np.abs(c.coords[3] - (x3 - np.floor(x3 / case.box) * case.box)).max() < 1e-15
    d = case.oracle(np.float64); x0 = d.coords[3].copy(); R.overdamped_run(d, 3, 0.0005, KB * 85.0, 50.0, key=1, ctr1=2)
    assert np.array_equal(d.coords[3], x0) and np.abs(d.coords - case.coords).max() > 1e-4


# ---- (b) the plan ------------------------------------------------------------------------------------------------------------------------------
def _expected_line(s, dt):
    P = R.plan(s, dt)
    k, oidx = 0, []
    for c in s:
        oidx.append(str(k) if c == "O" else "-"); k += c == "O"
    segs = ",".join("%d-%d:%d%d%d%d" % (b, e, P["force"][b], "A" in s[b:e], "B" in s[b:e], "O" in s[b:e]) for b, e in P["segments"])
    return "ok %s known=%d n_o=%d n_force=%d dts=%s force=%s oidx=%s seg=%s" % (
        s, P["forces_known_at_start"], s.count("O"), sum(P["force"]), ",".join(repr(float(d)) for d in P["dts"]), ",".join(str(int(f)) for f in P["force"]),
        ",".join(oidx), segs)


def test_plan_splitting_against_the_reference_rule(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "splitting_check.cpp")
    assert [l for l in open(src).read().splitlines() if l.startswith("#include \"")] == ['#include "splitting.h"']
    header = open(os.path.join(CSRC, "splitting.h")).read()
    assert [l for l in header.splitlines() if l.startswith("#include")] == ["#include <cstdint>"]      # host-only: no HIP header, nothing of the engine
    exe = tmp_path / "splitting_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    got = {l.split()[1]: l for l in lines if l.startswith("ok ")}
    strings = ["".join(t) for n in range(1, 7) for t in itertools.product("ABO", repeat=n)]
    assert len(strings) == 1092 and "strings: 1092" in lines
    for s in strings + ["BAOABBAOABBAOABB"]:
        want = _expected_line(s, 0.002)
        g = got[s]
        # the time steps as numbers (%.17g and repr both round-trip), everything else as text
        gd = [float(v) for v in re.search(r"dts=(\S+)", g).group(1).split(",")]; wd = [float(v) for v in re.search(r"dts=(\S+)", want).group(1).split(",")]
        assert gd == wd, (s, gd, wd)
        assert re.sub(r"dts=\S+", "", g) == re.sub(r"dts=\S+", "", want), (g, want)
    for label in ("null", "empty", "seventeen", "lowercase", "other"):
        assert "bad " + label in lines, label


def test_the_issue_table_of_force_computing_b():
    """the worked examples of the rule: which B computes forces, and whether the forces are known at the start"""
    want = {"BAOAB": (True, [4]), "OBABO": (True, [3]), "ABOBA": (False, [1]), "BAOA": (False, [0]), "BABAB": (True, [2, 4]), "AO": (True, []), "OOA": (True, [])}
    for s, (known, where) in want.items():
        P = R.plan(s, 0.002)
        assert P["forces_known_at_start"] == known and [j for j, f in enumerate(P["force"]) if f] == where, s
    assert R.plan("OOA", 0.003)["dts"] == [0.0015, 0.0015, 0.003] and R.plan("BAOAB", 0.002)["segments"] == [(0, 4), (4, 5)]
    with pytest.raises(ValueError):
        R.plan("BAoAB", 0.002)


# ---- (c) the ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_both_entry_points(pkg):
    import ctypes as C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mollyhip.h")).read(), flags=re.S)
    for name, n_args in (("mhip_splitting_run", 10), ("mhip_overdamped_run", 9)):
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n_args, name
        res, args = pkg.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == n_args
        assert getattr(pkg.lib(), name) is not None
    assert pkg.SIGNATURES["mhip_splitting_run"][1][6] is C.c_char_p
    assert pkg.lib().mhip_splitting_run(None, 0, 1, 0.002, 1.0, 1.0, b"BAOAB", 1, 1, 2) == -1      # null context
    assert pkg.lib().mhip_overdamped_run(None, 0, 1, 0.002, 1.0, 1.0, 1, 1, 2) == -1
    abi = open(os.path.join(ROOT, "julia", "ext", "mhip_abi.jl")).read()
    assert "(:mhip_splitting_run, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Cstring, Int32, UInt64, UInt64)" in abi
    assert "(:mhip_overdamped_run, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Int32, UInt64, UInt64)" in abi
    sim = pkg.LangevinSplitting(dt=0.002, temperature=300.0, friction=1.0, splitting="BAOAB")
    assert sim.remove_CM_motion == 1 and sim.coupling is None and pkg.OverdampedLangevin(dt=0.002, temperature=300.0, friction=1.0).remove_CM_motion == 1
    s = pkg.System(coords=np.zeros((4, 3)), boundary=pkg.CubicBoundary(2.0), pairwise_inters=(pkg.LennardJones(),))
    with pytest.raises(pkg.MollyHipError):      # only AndersenThermostat couples
        pkg.simulate(s, pkg.LangevinSplitting(0.002, 300.0, 1.0, "BAOAB", coupling=pkg.BerendsenThermostat(300.0, 0.1)), 1)
