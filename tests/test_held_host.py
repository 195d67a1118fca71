"""What the context holds and which call voids which part of it (molly.jl_amd/csrc/held.h) is host-only: tests/host/held_check.cpp includes
nothing but that header, checks every event's known answers — the full flag vector before and after, from at least two starting states —
and sweeps all 32 768 flag combinations × all events for the properties the engine relies on (who may turn the forces on, who clears
stale, what a voiding call leaves, the columns an event may touch).  No GPU, no library: the program is compiled here and must exit with status 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_held_known_answers_and_exhaustive_sweep(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "held_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "held.h"']
    header = open(os.path.join(ROOT, "molly.jl_amd", "csrc", "held.h")).read()
    assert [l for l in header.splitlines() if l.startswith("#include")] == []      # host-only: no HIP header, nothing of the engine
    exe = tmp_path / "held_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "molly.jl_amd", "csrc"), src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "sweep: 32768 states x 43 events" in run.stdout
    assert "held_check: all passed" in run.stdout


def test_engine_changes_the_flags_through_events_only():
    """engine.hip declares none of the flags and assigns none of them: it holds one Held and calls its events."""
    import re
    text = open(os.path.join(ROOT, "molly.jl_amd", "csrc", "engine.hip")).read()
    flags = ("stale coords_moved export_needs_search inner_valid prune_disp_exceeded frc_valid frc_run_total frc_before_set_state "
             "state_set params_set state_pending vel_check_due trk_issued prune_pending interior_done").split()
    raw = re.findall(r"(?<![\w.])(?:%s)\s*(?:=(?!=)|\|=|&=)" % "|".join(flags), text)
    assert raw == [], raw
    assert len(re.findall(r"^\s*Held held;", text, re.M)) == 1
