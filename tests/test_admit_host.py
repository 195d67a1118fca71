"""Which call a context admits in its present configuration (molly.jl_amd/csrc/admit.h) is host-only: tests/host/admit_check.cpp includes nothing but
that header, checks every entry's known answers — the state of exactly its needs, each single mode added, each single need removed, transcribed by
hand from the header's table — and sweeps all 262 144 mode combinations × all entries for the properties the header lists (an integrator that ignores
a feature refuses it, exclusions are symmetric, no excluded pair is reachable, no entry refuses its own needs, a verdict reads only the columns its
row names).  No GPU, no library: the program is compiled here and must exit with status 0."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "molly.jl_amd", "csrc", "engine.hip")


def test_admit_known_answers_and_exhaustive_sweep(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "admit_check.cpp")
    text = open(src).read()
    assert [l for l in text.splitlines() if l.startswith("#include \"")] == ['#include "admit.h"']
    header = open(os.path.join(ROOT, "molly.jl_amd", "csrc", "admit.h")).read()
    assert [l for l in header.splitlines() if l.startswith("#include")] == ["#include <cstdint>"]      # host-only: no HIP header, nothing of the engine
    exe = tmp_path / "admit_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "molly.jl_amd", "csrc"), src, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "sweep: 262144 states x 38 entries" in run.stdout
    assert "admit_check: all passed" in run.stdout


def test_engine_refuses_through_the_table_only():
    """no UNSUPPORTED / STATE throw of engine.hip reads the configuration itself: the refusals that are left depend on the data handed over"""
    reads = ("con_on", "vs_on", "thermo_on()", "andersen_prob", "tri_mode", "hp_set", "dom.ready", "xf.world", "held.state_set()", "held.params_set()")
    bad = [l.strip() for l in open(ENGINE).read().splitlines()
           if ("throw ApiError{MHIP_ERR_UNSUPPORTED" in l or "throw ApiError{MHIP_ERR_STATE" in l) and any(r in l for r in reads)]
    assert bad == [], bad


# the overrides that are entries of the table (the two lazy checks sit in helpers: rebuild_impl, step_forces)
ENTRY_OVERRIDES = ("vv_run langevin_run vv_init vv_stage1 vv_stage2 halo_start halo_mid halo_begin halo_end halo_end_parts domain_run redraw_velocities "
                   "tune_launch set_box constraint_virial place_virtual_sites distribute_forces specific_forces specific_virial specific_potential_energy "
                   "general_forces general_virial general_potential_energy set_halo_routes halo_open_peer halo_selftest domain_export "
                   "set_atom_counts set_domain halo_region set_triclinic set_constraints set_virtual_sites set_thermostat set_andersen set_halo_plan").split()


def method_body(text, start):
    """the text of the member function that starts at `start`: one line, or up to the closing brace at the class's indentation"""
    line = text[start:text.index("\n", start)]
    return line if line.rstrip().endswith("}") else text[start:text.index("\n    }\n", start)]


def test_every_entry_point_asks_the_table():
    text = open(ENGINE).read()
    assert len(re.findall(r"^\s*uint32_t modes\(\) const \{", text, re.M)) == 1
    assert len(re.findall(r"^\s*void admit\(adm::Entry", text, re.M)) == 1
    for name in ENTRY_OVERRIDES:
        found = list(re.finditer(r"^    [\w:<>\*& ]+?\b%s\([^;{]*\) (?:const )?override \{" % name, text, re.M))
        assert len(found) == 1, name
        assert "admit(adm::" in method_body(text, found[0].start()), name
    # the helpers the step loops use ask nothing
    for helper in ("stage1_impl", "init_impl", "halo_mid_impl", "halo_start_impl", "redraw_impl", "place_sites", "vv_loop"):
        found = list(re.finditer(r"^    \w+ %s\([^;{]*\) \{" % helper, text, re.M))
        assert len(found) == 1, helper
        assert "admit(" not in method_body(text, found[0].start()), helper
    assert "constrained()" not in text and "has_sites()" not in text and "!in_run" not in text
