"""The pair-list validity policy (molly.jl_amd/csrc/list_policy.h) is host-only arithmetic: tests/host/list_policy_check.cpp includes
nothing but that header, checks the decision's known answers in every call form and sweeps 200 000 seeded inputs for the safety
property the rule exists for.  No GPU, no library: the program is compiled here and must exit with status 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_policy_known_answers_and_safety_sweep(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "list_policy_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "list_policy.h"']
    exe = tmp_path / "list_policy_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "molly.jl_amd", "csrc"), src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "sweep: 200000 inputs" in run.stdout
