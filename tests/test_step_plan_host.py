"""Which launch closes an MD step, what the force pass is asked to do on the way, how many blocks the launch gets and where its Σ m v partials go
(molly.jl_amd/csrc/step_plan.h) is host-only arithmetic: tests/host/step_plan_check.cpp includes nothing but that header, checks the known answers of
every launch form at the edges of a run — first and last step, thermostat steps, cadence steps with and without the dual list, a check already issued,
caller parts, the clamps of the block rules — and sweeps every combination of the boolean fields × loops × step positions × atom counts for the
properties the engine relies on.  No GPU, no library: the program is compiled here and must exit with status 0."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molly.jl_amd", "csrc")


def test_step_plan_known_answers_and_sweep(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "step_plan_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "step_plan.h"']
    header = open(os.path.join(CSRC, "step_plan.h")).read()
    assert [l for l in header.splitlines() if l.startswith("#include")] == ["#include <algorithm>", "#include <cstdint>"]      # host-only: no HIP header, nothing of the engine
    exe = tmp_path / "step_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    # 3 loops x 128 run shapes x 6 step positions x 8 x 3 x 3 x 2 step fields x 14 atom counts
    assert "sweep: %d step shapes" % (3 * 128 * 6 * 8 * 3 * 3 * 2 * 14) in run.stdout
    assert "step_plan_check: all passed" in run.stdout


def test_engine_takes_the_step_schedule_from_the_plan():
    """engine.hip writes out neither block rule, keeps no per-loop mode flags, and asks whether a launch may measure a check in one place: the helper that fills a StepShape."""
    text = open(os.path.join(CSRC, "engine.hip")).read()
    for gone in ("n_owned / 2048", "cdiv(n_owned, 256), 1024)", "in_vv_fused", "in_lang_fused", "in_lang_async"):
        assert gone not in text, gone
    helper = re.search(r"^    StepShape step_shape\(.*?^    }\n", text, re.M | re.S)
    assert helper and "async_ok()" in helper.group(0) and "held.trk_issued()" in helper.group(0)
    rest = text.replace(helper.group(0), "")
    assert re.search(r"async_ok\(\)\s*&&\s*!held\.trk_issued\(\)", rest) is None
    assert len(re.findall(r"^\s*RunPlan run;", text, re.M)) == 1
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^\$\(BUILD\)/engine\.o:.*\bstep_plan\.h\b", makefile, re.M)
