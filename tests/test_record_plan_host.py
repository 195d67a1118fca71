"""At which steps of a run the recorder fires, for which channels, how many records a run makes and whether they fit (molly.jl_amd/csrc/record_plan.h)
is host-only arithmetic: tests/host/record_plan_check.cpp includes nothing but that header, checks the known answers at the edges — a record at the run's
last step, none in a run shorter than the interval, a record step equal to `first`, all channels off, intervals 1 and 2^31 − 1 — and sweeps firsts ×
lengths × interval quadruples × used / capacity against a brute-force loop over the steps.  No GPU, no library: the program is compiled here with the
address and undefined-behaviour sanitizers and must exit with status 0."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molly.jl_amd", "csrc")


def test_record_plan_known_answers_and_sweep(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "record_plan_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "record_plan.h"']
    header = open(os.path.join(CSRC, "record_plan.h")).read()
    assert [l for l in header.splitlines() if l.startswith("#include")] == ["#include <algorithm>", "#include <cstdint>"]      # host-only: no HIP header, nothing of the engine
    exe = tmp_path / "record_plan_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    # 12 firsts x 10 lengths x 8 x 8 x 4 x 3 interval quadruples x 15 (used <= capacity) pairs
    assert "sweep: %d cases" % (12 * 10 * 8 * 8 * 4 * 3 * 15) in run.stdout
    assert "record_plan_check: all passed" in run.stdout


def test_engine_takes_the_record_steps_from_the_plan():
    """engine.hip walks a recorded run by rec_next_step / rec_mask and refuses by rec_fits: it writes out no modulus of its own over the intervals"""
    text = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "record_plan.h"' in text
    for used in ("rec_next_step(", "rec_mask(", "rec_fits("):
        assert used in text, used
    assert re.search(r"%\s*rec\w*\.every", text) is None
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^\$\(BUILD\)/engine\.o:.*\brecord_plan\.h\b.*\brecord\.h\b|^\$\(BUILD\)/engine\.o:.*\brecord\.h\b.*\brecord_plan\.h\b", makefile, re.M)
