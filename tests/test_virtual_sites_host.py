"""Virtual sites without a GPU: the numpy reference (tests/virtual_sites_ref.py) against the reference's known answers
(tests/golden/virtual_sites_basic.json), the Python mirror's constructors and refusals, the C ABI declarations, the four-site water
start, and the compiled k_con_step holding no more scratch memory than before it hosted sites."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import virtual_sites_ref as V
from tests import systems as S  # noqa: F401  (Case.oracle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molly.jl_amd", "csrc")
ENTRY_POINTS = ("mhip_set_virtual_sites", "mhip_place_virtual_sites", "mhip_distribute_forces", "mhip_virtual_site_info")


def mod():
    import molly_loader
    return molly_loader.load()


def test_reference_reproduces_the_known_answers():
    """the bars of the reference's own test: 1e-10 nm, 1e-10 relative, 1e-9 and 1e-10 kJ/mol/nm"""
    g = V.toy()
    x = V.place(g["coords"], g["box"], g["sites"])
    assert np.linalg.norm(x - g["coords_true"], axis=1).max() < 1e-10
    raw, pe = V.lj_all_pairs(x, g["box"], g["sigma"], g["eps"], g["excluded"])
    assert abs(pe - g["potential_energy"]) <= 1e-10 * abs(g["potential_energy"])
    f = V.distribute(raw, x, g["box"], g["sites"])
    assert np.linalg.norm(f - g["fs_true"], axis=1).max() < 1e-9
    assert np.linalg.norm(f.sum(0)) < 1e-10
    assert not f[g["flags"]].any() and raw[g["flags"]].any()
    assert np.array_equal(V.flags(len(x), g["sites"]), g["flags"])


def test_reference_distribution_conserves_force_and_torque():
    """the transposed Jacobian by finite differences: f_site · δr_site = Σ F_parent · δr_parent for every site type"""
    g = V.toy()
    rng = np.random.default_rng(0)
    x = V.place(g["coords"], g["box"], g["sites"])
    for site in g["sites"]:
        s = site[1]
        fs = rng.normal(size=3)
        f = np.zeros_like(x); f[s] = fs
        F = V.distribute(f, x, g["box"], [site])
        for a in [p for p in site[2:5] if p >= 0]:
            for d in range(3):
                h = 1e-6
                xp = x.copy(); xp[a, d] += h
                xm = x.copy(); xm[a, d] -= h
                dr = (V.place(xp, g["box"], [site])[s] - V.place(xm, g["box"], [site])[s]) / (2 * h)
                assert abs(fs @ dr - F[a, d]) < 1e-8


def test_constructors_and_refusals_of_the_mirror():
    m = mod()
    with pytest.raises(ValueError):
        m.TwoParticleAverageSite(2, 0, 1, 0.6, 0.5)
    with pytest.raises(ValueError):
        m.ThreeParticleAverageSite(6, 3, 4, 5, 0.3, 0.3, 0.5)
    a = m.TwoParticleAverageSite(2, 0, 1, 0.6, 0.4)
    assert (a.type, a.atom_ind, a.atom_1, a.atom_2, a.atom_3, a.weights) == (2, 2, 0, 1, -1, (0.6, 0.4, 0.0, 0.0, 0.0, 0.0))
    b = m.OutOfPlaneSite(10, 7, 8, 9, 0.4, 0.4, 0.2)
    assert b.type == 4 and b.weights == (0.0, 0.0, 0.0, 0.4, 0.4, 0.2)
    assert m.OneParticleSite(12, 0).type == 1 and m.ThreeParticleAverageSite(6, 3, 4, 5, 0.2, 0.3, 0.5).type == 3
    g = V.toy()
    s = V.toy_case(g).system(m, np.float64)
    assert np.array_equal(s.virtual_site_flags, g["flags"]) and len(s.virtual_sites) == 5
    x = np.zeros((4, 3)); box = m.CubicBoundary(3.0)
    with pytest.raises(ValueError):      # the same atom defined twice
        m.System(coords=x, boundary=box, virtual_sites=(m.OneParticleSite(3, 0), m.OneParticleSite(3, 1)))
    with pytest.raises(ValueError):      # a parent that is a site
        m.System(coords=x, boundary=box, virtual_sites=(m.OneParticleSite(3, 0), m.OneParticleSite(2, 3)))
    with pytest.raises(ValueError):      # out of range
        m.System(coords=x, boundary=box, virtual_sites=(m.OneParticleSite(4, 0),))
    with pytest.raises(ValueError):      # a site in a constraint
        m.System(coords=x, boundary=box, virtual_sites=(m.OneParticleSite(3, 0),),
                 constraints=(m.SHAKE_RATTLE(4, dist_constraints=[m.DistanceConstraint(2, 3, 0.1)]),))
    # what stays in Julia: refused before any engine call
    with pytest.raises(m.MollyHipError):
        m.simulate(s, m.SteepestDescentMinimizer())
    with pytest.raises(m.MollyHipError):
        m.scale_coords(s, np.eye(3) * 1.01)
    with pytest.raises(m.MollyHipError):
        m.simulate(s, m.VelocityVerlet(dt=0.001, coupling=m.MonteCarloBarostat(1.0, 300.0, s.boundary)), 1)
    with pytest.raises(m.MollyHipError, match="OutOfPlaneSite"):
        m.virial(s)
    with pytest.raises(m.MollyHipError, match="OutOfPlaneSite"):
        m.pressure(s)


def test_header_and_signatures_declare_the_entry_points():
    m = mod()
    header = open(os.path.join(ROOT, "include", "mollyhip.h")).read()
    assert "virtual sites (src/virtual.jl)" in header
    for name in ENTRY_POINTS:
        assert re.search(r"int32_t\s+" + name + r"\(mhip_ctx\* ctx", header), name
        assert name in m.SIGNATURES
    assert len(m.SIGNATURES["mhip_set_virtual_sites"][1]) == 8 and len(m.SIGNATURES["mhip_distribute_forces"][1]) == 3


def test_case_field_defaults_to_no_sites():
    from molly_jl_amd.workloads import Case, lj_fluid
    assert Case(np.zeros((2, 3)), 3.0).virtual_sites == ()
    assert lj_fluid(4).virtual_sites == ()


def test_tip4p_box_start():
    w = V.tip4p_fb()
    case = V.tip4p_box(6)
    assert case.n == 4 * 216 and len(case.virtual_sites) == 216 and len(case.excluded) == 6 * 216
    assert V.min_intermolecular_distance(case) >= 0.12
    x, box = case.coords, case.box
    o, h1, h2, ms = x[0::4], x[1::4], x[2::4], x[3::4]
    mi = V.CR.min_image
    assert np.abs(np.linalg.norm(mi(h1 - o, box), axis=1) - w["bond_length"]).max() < 1e-12
    assert np.abs(np.linalg.norm(mi(h1 - h2, box), axis=1) - case.d_hh).max() < 1e-12
    assert np.abs(np.linalg.norm(mi(ms - o, box), axis=1) - 0.010527).max() < 2e-6      # the O–M distance of TIP4P-FB, 0.10527 Å
    assert np.abs(mi(V.place(x, box, case.virtual_sites) - x, box)).max() == 0.0
    assert abs(case.charge.sum()) < 1e-9 and not case.mass[3::4].any() and not case.velocities[3::4].any()
    three = V.tip4p_box(6, three_site=True)
    assert three.n == 3 * 216 and three.virtual_sites == () and abs(three.charge.sum()) < 1e-9
    assert np.array_equal(three.coords, np.delete(x, np.arange(3, case.n, 4), axis=0))
    flex = V.tip4p_box(6, rigid=False)
    assert flex.constraints is None and len(flex.bonds["i"]) == 432 and len(flex.angles["i"]) == 216


# k_con_step of the commit before sites were hosted (ed82a24), `tools/kernel_resources.py` on constraints.hip compiled with the flags below:
# scratch bytes per lane of the eight instantiations (precision, mode)
PARENT_SCRATCH = {("float", 0): 0, ("float", 1): 0, ("float", 2): 0, ("float", 3): 0, ("double", 0): 0, ("double", 1): 0, ("double", 2): 0, ("double", 3): 0}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_con_step_holds_no_more_scratch_than_before(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "constraints.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "constraints.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    table = subprocess.run(["python3", os.path.join(ROOT, "tools", "kernel_resources.py"), str(out), "--filter", "k_con_step"],
                           check=True, capture_output=True, text=True).stdout
    found = {}
    for line in table.splitlines():
        mt = re.match(r"\s*(\d+)\s+\d+\s+\d+\s+\d+\s+(\d+)\s+.*k_con_step<(float|double), (\d)>", line)
        if mt:
            found[(mt.group(3), int(mt.group(4)))] = (int(mt.group(1)), int(mt.group(2)))
    assert set(found) == set(PARENT_SCRATCH), table
    for k, (scratch, n_instr) in found.items():
        assert scratch <= PARENT_SCRATCH[k] and n_instr == 0, (k, scratch, n_instr)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_spread_uses_hardware_float_atomics(tmp_path):
    """several sites may share a parent: k_vs_spread adds with one global_atomic_add_f32 / _f64 per component, no compare-and-swap loop, and neither
    one-shot kernel touches scratch memory"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "virtual_sites.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "virtual_sites.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    text = open(out).read()
    assert text.count(".amdhsa_kernel") == 4
    assert text.count("global_atomic_add_f32") == 9 and text.count("global_atomic_add_f64") == 9
    assert "cmpswap" not in text and not re.search(r"^\s+scratch_", text, flags=re.M)
