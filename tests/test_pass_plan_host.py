"""Which pair pass runs, and with what LDS (molly.jl_amd/csrc/pass_plan.h), is host-only arithmetic: tests/host/pass_plan_check.cpp includes
nothing but that header, checks the plan's known answers — stride bands, segmentation edges, the prune reserve, the group-split bound, who
may integrate — and sweeps 200 000 seeded shapes for the layout properties every launch relies on (among them: the packed pruning kernel's
compile-time table offset is where the plan puts the table).  No GPU, no library: the program is compiled here and must exit with status 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_plan_known_answers_and_layout_sweep(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "pass_plan_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "pass_plan.h"']
    exe = tmp_path / "pass_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "molly.jl_amd", "csrc"), src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "sweep: 200000 inputs" in run.stdout
