"""The rescaling thermostats' scale factor (molly.jl_amd/csrc/thermostat.h) is host+device arithmetic on a handful of doubles:
tests/host/thermostat_check.cpp includes nothing but that header and checks the three kinds against closed forms, the identities between
them (Berendsen with τ = dt is Immediate; CSVR with c → 0 and with τ → ∞), the guards, and the centre-of-mass identity of the kinetic
energy against an explicit sum.  No GPU, no library: the program is compiled here and must exit with status 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thermostat_lambda_known_answers_identities_and_guards(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "thermostat_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "thermostat.h"']
    header = open(os.path.join(ROOT, "molly.jl_amd", "csrc", "thermostat.h")).read()
    assert sorted(l.split()[1] for l in header.splitlines() if l.startswith("#include")) == ["<cmath>", "<cstdint>"]
    exe = tmp_path / "thermostat_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "molly.jl_amd", "csrc"), src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "sweep: 200 seeded velocity sets" in run.stdout and "all thermostat checks passed" in run.stdout
