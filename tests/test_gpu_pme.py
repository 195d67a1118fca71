"""HIP PME reciprocal space (csrc/pme.h) against the oracle restatement and the OpenMM fixtures of the reference
(test/protein.jl:208-299)."""
import numpy as np
import pytest

from tests import golden6mrr as G
from tests import systems as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,order,box_scale,mesh", [(np.float64, 5, (1.0, 1.0, 1.0), None), (np.float64, 4, (1.0, 1.15, 1.3), (14, 17, 21)),
                                                       (np.float64, 6, (1.0, 1.0, 1.0), (16, 12, 15)), (np.float32, 5, (1.0, 1.1, 1.0), None)])
def test_reciprocal_forces_and_energy_vs_oracle(pkg, dtype, order, box_scale, mesh):
    pme = dict(order=order, error_tol=5e-4)
    if mesh:
        pme["mesh"] = mesh
    case = S.charged_fluid(10, dict(kind="ewald", rc=1.0, tol=5e-4), dtype=dtype, pme=pme, box_scale=box_scale, with_exceptions=False)
    o = case.oracle(np.float64)
    f_ref = o.forces(None, pairwise=False, specific=False, general=True)
    e_ref = o.potential_energy(None, pairwise=False, general=True)
    s = case.system(pkg, dtype)
    f = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    e = pkg.potential_energy(s, pairwise=False, specific=False)
    scale = np.linalg.norm(f_ref, axis=1).max()
    rel_f, rel_e = (1e-10, 1e-11) if dtype == np.float64 else (2e-4, 2e-5)     # fp32: spread atomics + 50-term DFT sums in single precision
    assert np.linalg.norm(f - f_ref, axis=1).max() < rel_f * scale
    assert abs(e - e_ref) < rel_e * abs(e_ref)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reciprocal_forces_with_a_charge_beyond_the_fixed_point_range(pkg, dtype):
    """the spreading kernel accumulates its LDS sub-mesh in fixed point (2^28 per unit of q·w in fp32: |q| < 26); a batch holding a larger
    charge must take the direct path and still be right"""
    case = S.charged_fluid(8, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=dtype, pme=dict(order=5, error_tol=5e-4), r_list=1.0, with_exceptions=False)
    q = np.array(case.charge, dtype=np.float64)
    q[7] += 40.0; q[300] -= 40.0                                              # two ions far beyond the range, neutral in sum
    case.charge = q.astype(dtype).astype(np.float64)
    o = case.oracle(np.float64)
    f_ref = o.forces(None, pairwise=False, specific=False, general=True)
    s = case.system(pkg, dtype)
    f = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    scale = np.linalg.norm(f_ref, axis=1).max()
    assert np.linalg.norm(f - f_ref, axis=1).max() < (1e-10 if dtype == np.float64 else 2e-4) * scale


def test_6mrr_reciprocal_fp32_vs_fp64_oracle(pkg):
    case = G.case("ewald", np.float32, bonded=False, lj=False, pme=True)
    o = case.oracle(np.float64)
    f_ref = o.forces(None, pairwise=False, specific=False, general=True)
    s = case.system(pkg, np.float32)
    f = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    err = np.linalg.norm(f - f_ref, axis=1)
    assert err.max() < 2e-4 * np.linalg.norm(f_ref, axis=1).max()
    assert np.sqrt((err ** 2).mean()) < 2e-5 * np.sqrt((f_ref ** 2).sum(axis=1).mean())
    e_ref = o.potential_energy(None, pairwise=False, general=True)
    assert abs(pkg.potential_energy(s, pairwise=False, specific=False) - e_ref) < 2e-5 * abs(e_ref)


@pytest.mark.parametrize("exact,ftol,etol", [(True, 1e-6, 1e-4), (False, 1e-3, 0.2)])
def test_all_pme_vs_openmm_fp64(pkg, exact, ftol, etol):
    """the reference's bars (test/protein.jl:267, 274): 1e-7 / 1e-5 with exact erfc, 1e-3 / 0.2 with the A&S approximation; the
    exact case is held to 1e-6 / 1e-4 here (other summation orders than OpenMM's, forces of 1e4 kJ/mol/nm)"""
    d = G.data()
    case = G.case("ewald", np.float64, bonded=True, approx_erfc=not exact, pme=True)
    s = case.system(pkg, np.float64)
    key = "all_pme_exact" if exact else "all_pme"
    f = pkg.forces(s)
    assert np.linalg.norm(f - d[f"openmm_forces_{key}"], axis=1).max() < ftol
    e = pkg.potential_energy(s) + G.lj_dispersion_correction(d)
    assert abs(e - float(d[f"openmm_energy_{key}"])) < etol


def test_100_step_pme_trajectory_vs_openmm_fp64(pkg):
    """test/protein.jl:278-299 on the device: the complete MD step (pair + bonded + PME + integrator)"""
    d = G.data()
    case = G.case("ewald", np.float64, bonded=True, approx_erfc=False, pme=True)
    s = case.system(pkg, np.float64)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 100)
    xo = d["openmm_coordinates_100steps"]; box = case.box
    dx = s.coords - (xo - np.floor(xo / box) * box)
    dx -= np.round(dx / box) * box
    assert np.linalg.norm(dx, axis=1).max() < 1e-9                                            # reference bar 1e-10 (same summation order as OpenMM's CPU platform)
    assert np.linalg.norm(s.velocities - d["openmm_velocities_100steps"], axis=1).max() < 1e-7


def test_all_pme_fp32_total_force_vs_openmm(pkg, slack):
    """The configuration bench.py TIMES (6mrr_pme: Float32, LJ + Ewald direct space with the A&S erfc + bonded + EwaldExclusion + PME
    reciprocal space) as ONE force evaluation against OpenMM's forces_all_pme.txt.
    Two parts, because two things separate an fp32 engine from that file.  (a) The INPUTS: coordinates rounded to fp32 (ulp/2 = 2.4e-7 nm
    at 5 nm) under bond constants of 4e5 kJ mol⁻¹ nm⁻² move a force by ≈ 0.1 per bond whatever the arithmetic — the fp64 oracle on the
    rounded inputs is 0.31 kJ mol⁻¹ nm⁻¹ off OpenMM at the worst atom (on forces of up to 6 300).  (b) The ARITHMETIC: the engine against
    that fp64 oracle on the same rounded inputs, per atom within the fp32 pair bar 4e-5·Σ_j‖f_ij‖ (tests/systems.py) + 5e-6 of the atom's
    bonded force scale + 5e-5 of the largest reciprocal-space force (fp32 mesh sums) + 2.5e-4.  Round 4 allowed four times each of the three
    add-ons; the recorded slack (the `slack` fixture) showed the worst atom at 0.36 of that bar and — at 0.76 — inside the PAIR bar
    alone, so they were cut to a quarter.  Against OpenMM itself: (a) + (b) per atom, 0.5 kJ mol⁻¹ nm⁻¹ at the worst atom (measured 0.31: the
    input rounding), relative RMS 2e-5 (measured 1.6e-5).  Energy: the reference's approximate-erfc bar 0.2 kJ/mol (test/protein.jl:274) + 5e-7
    of Σ|e_ij| ≈ 6e5 in fp32 (measured 0.26)."""
    d = G.data()
    case = G.case("ewald", np.float32, bonded=True, pme=True)                 # approximate_erfc = True: the default, and what is timed
    tol, o, nl = S.fp32_force_tolerance(case)
    bonded_scale = np.linalg.norm(o.forces(None, pairwise=False, specific=True), axis=1)
    pme_scale = np.linalg.norm(o.forces(None, pairwise=False, specific=False, general=True), axis=1).max()
    f_ref = o.forces(nl, nthreads=8, specific=True, general=True)             # fp64 arithmetic on the fp32-rounded inputs
    f_omm = d["openmm_forces_all_pme"]
    input_term = np.linalg.norm(f_ref - f_omm, axis=1)
    assert input_term.max() < 0.5
    s = case.system(pkg, np.float32)
    f = pkg.forces(s).astype(np.float64)
    bar = tol + 5e-6 * bonded_scale + 5e-5 * pme_scale + 2.5e-4
    err = np.linalg.norm(f - f_ref, axis=1)
    w = int((err / bar).argmax())
    slack(f"arithmetic: worst per-atom error / bar (atom {w}: pair part {tol[w]:.3g}, bonded part {5e-6 * bonded_scale[w]:.3g}, mesh part {5e-5 * pme_scale:.3g}, constant 2.5e-4)", (err / bar).max(), 1.0)
    slack("arithmetic: worst per-atom error against the pair bar ALONE (how much the other three allowances are needed)", (err / tol).max(), (bar / tol).max())
    err_omm = np.linalg.norm(f - f_omm, axis=1)
    slack("against OpenMM: worst per-atom error / (bar + input rounding)", (err_omm / (bar + input_term)).max(), 1.0)
    slack("against OpenMM: worst per-atom error, kJ/mol/nm", err_omm.max(), 0.5)
    slack("against OpenMM: relative RMS", S.rel_rms(err_omm, f_omm), 2e-5)
    e = pkg.potential_energy(s) + G.lj_dispersion_correction(d)
    slack("potential energy against OpenMM, kJ/mol", abs(e - float(d["openmm_energy_all_pme"])), 0.2 + 0.3)


def test_100_step_pme_trajectory_vs_openmm_fp32(pkg, slack):
    """test/protein.jl:278-299 with the timed configuration's arithmetic (Float32, approximate erfc, the complete MD step) through
    mhip_vv_run: 100 steps of 0.5 fs from OpenMM's start velocities against coordinates_100steps.txt.  SURVEY §8(c)'s fp32 trajectory bar is
    5e-4 nm per atom (test/simulation.jl:625); the recorded slack showed 1.7e-5 nm at the worst atom, 1.8e-6 nm on average and
    2.8e-3 nm/ps in the velocities (hydrogens move at ≈ 3), so the test holds 5e-5 nm, 5e-6 nm and 8e-3 nm/ps — a tenth of the reference's bar."""
    d = G.data()
    case = G.case("ewald", np.float32, bonded=True, pme=True)
    s = case.system(pkg, np.float32)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 100)
    st = s.stats()
    # the timed path itself: the group-split pair pass with spreading and bonded terms in its launch, and the step's last launch integrating (k_gather_collect_vv)
    assert st["n_fused_steps"] > 60 and st["n_group_split_passes"] > 60, (st["n_fused_steps"], st["n_group_split_passes"])
    xo = d["openmm_coordinates_100steps"]; box = case.box
    dx = s.coords.astype(np.float64) - (xo - np.floor(xo / box) * box)
    dx -= np.round(dx / box) * box
    dev = np.linalg.norm(dx, axis=1)
    slack("worst coordinate deviation after 100 steps, nm", dev.max(), 5e-5)
    slack("mean coordinate deviation after 100 steps, nm", dev.mean(), 5e-6)
    slack("worst velocity deviation after 100 steps, nm/ps", np.linalg.norm(s.velocities.astype(np.float64) - d["openmm_velocities_100steps"], axis=1).max(), 8e-3)


def test_pme_rejects_what_it_does_not_cover(pkg):
    case = S.charged_fluid(6, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=np.float32, pme=dict(order=7), r_list=0.9, with_exceptions=False)
    with pytest.raises(pkg.MollyHipError):
        pkg.forces(case.system(pkg, np.float32), pairwise=False)


def test_complete_pme_step_conserves_energy_fp64(pkg):
    """NVE with every interaction incl. reciprocal PME (Float64, dt 0.5 fs, remove_CM_motion = 0): forces and energies of the
    direct, reciprocal and exclusion parts belong to one Hamiltonian — the total energy stays bounded and returns at equal phase of
    the O-H ringing (same bars as the reaction-field run of test_gpu_6mrr.py)."""
    case = G.case("ewald", np.float64, bonded=True, approx_erfc=False, pme=True)
    s = case.system(pkg, np.float64)
    e0 = pkg.total_energy(s)
    assert e0 + G.lj_dispersion_correction() == pytest.approx(96522.24858589929, abs=1e-3)     # test/protein.jl:285
    es = [e0]
    for k in range(10):
        pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005, remove_CM_motion=0), 20, init_step=20 * k)
        es.append(pkg.total_energy(s))
    assert max(abs(e - e0) for e in es) < 0.06 * abs(e0)
    assert abs(es[5] - e0) < 2e-3 * abs(e0) and abs(es[-1] - e0) < 5e-3 * abs(e0)


@pytest.mark.parametrize("dtype,rel", [(np.float64, 1e-9), (np.float32, 3e-4)])
def test_total_virial_and_pressure_6mrr_vs_oracle(pkg, dtype, rel):
    """virial(sys) = pairwise + specific + PME parts (energy.jl:116-131), each against the oracle; test/protein.jl:168-171:
    scalar_virial = tr(virial), scalar_pressure = tr(pressure) / 3"""
    case = G.case("ewald", dtype, bonded=True, approx_erfc=False, pme=True)
    o = case.oracle(np.float64)
    nl = o.neighbors("cell", nthreads=8)
    s = case.system(pkg, dtype)
    for kw in (dict(pairwise=True, specific=False, general=False), dict(pairwise=False, specific=True, general=False), dict(pairwise=False, specific=False, general=True)):
        w_ref = o.virial(nl, **kw)
        w = pkg.virial(s, **kw)
        assert np.abs(w - w_ref).max() < rel * np.abs(w_ref).max(), kw
    w = pkg.virial(s)
    assert np.abs(w - o.virial(nl, pairwise=True, specific=True, general=True)).max() < rel * np.abs(w).max()
    assert pkg.scalar_virial(s) == pytest.approx(np.trace(w), rel=rel)        # recomputed: the spread's atomics reorder the mesh sums
    p = pkg.pressure(s)
    k = 0.5 * np.einsum("i,ia,ib->ab", case.mass, case.velocities, case.velocities)
    assert np.abs(p - (2 * k + w) / np.prod(case.box)).max() < rel * np.abs(p).max()
    assert pkg.scalar_pressure(s) == pytest.approx(np.trace(p) / 3, rel=rel)


def _tri_pme_case(dtype, basis, mesh, n_side=9, stable=False):
    """the charged fluid of the other tests in a sheared cell: atoms keep their places, the cell gets the tilt"""
    case = S.charged_fluid(n_side, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=dtype, pme=dict(order=5, mesh=mesh), r_list=1.0, with_exceptions=False, stable=stable)
    L = float(case.box[0])
    bv = np.array(basis, dtype=np.float64) * L
    case.triclinic = dict(basis=bv.astype(dtype).astype(np.float64), approx_images=False)
    case.box = np.diag(case.triclinic["basis"]).copy()
    return case


@pytest.mark.parametrize("dtype,basis,mesh", [
    (np.float64, [[1, 0, 0], [0.3, 1, 0], [0.2, -0.25, 1]], (24, 24, 24)),        # even meshes: the Nyquist planes of a sheared cell (averaged influence function)
    (np.float64, [[1, 0, 0], [0.45, 1, 0], [-0.3, 0.4, 1]], (21, 22, 25)),
    (np.float32, [[1, 0, 0], [0.3, 1, 0], [0.2, -0.25, 1]], (24, 22, 26)),
    (np.float64, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], (24, 24, 24)),                # no tilt: the cubic numbers through the triclinic path
])
def test_triclinic_reciprocal_forces_and_energy_vs_oracle(pkg, dtype, basis, mesh):
    """PME on a TriclinicBoundary (recip_box of spatial.jl:338-347 in the placement, the wave vectors and the force transform; ewald.jl:486, 688-694, 846-849).
    The oracle visits the full mesh like the reference; the engine's half spectrum carries the mean of the influence function of k and −k where they
    differ (Nyquist planes of a sheared cell)."""
    case = _tri_pme_case(dtype, basis, mesh)
    o = case.oracle(np.float64)
    f_ref = o.forces(None, pairwise=False, specific=False, general=True)
    e_ref = o.potential_energy(None, pairwise=False, general=True)
    s = case.system(pkg, dtype)
    f = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    e = pkg.potential_energy(s, pairwise=False, specific=False)
    scale = np.linalg.norm(f_ref, axis=1).max()
    rel_f, rel_e = (1e-10, 1e-11) if dtype == np.float64 else (2e-4, 2e-5)
    assert np.linalg.norm(f - f_ref, axis=1).max() < rel_f * scale, np.linalg.norm(f - f_ref, axis=1).max() / scale
    assert abs(e - e_ref) < rel_e * abs(e_ref)
    # the reciprocal-space virial: every wave vector of the full mesh with its own m · recip_box (the mirror of a Nyquist index is not −m on a sheared cell)
    w = pkg.virial(s, pairwise=False, specific=False)
    w_ref = o.virial(None, pairwise=False, specific=False, general=True)
    assert np.abs(w - w_ref).max() < (1e-9 if dtype == np.float64 else 2e-4) * np.abs(w_ref).max()


def test_triclinic_ewald_total_forces_and_short_run_vs_oracle(pkg):
    """direct space (exact minimum image on the sheared cell) + reciprocal space together, and 20 velocity-Verlet steps of it"""
    case = _tri_pme_case(np.float64, [[1, 0, 0], [0.3, 1, 0], [0.2, -0.25, 1]], (24, 24, 24), stable=True)
    o = case.oracle(np.float64)
    nl = o.neighbors("brute")
    f_ref = o.forces(nl, pairwise=True, specific=False, general=True)
    s = case.system(pkg, np.float64)
    f = pkg.forces(s)
    assert np.linalg.norm(f - f_ref, axis=1).max() < 1e-9 * np.linalg.norm(f_ref, axis=1).max()
    o.vv_run(20, 0.0005, remove_cm_every=1, general=True)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 20)
    bv = case.triclinic["basis"]
    d = np.asarray(s.coords, dtype=np.float64) - o.coords
    d -= np.round(d @ np.linalg.inv(bv)) @ bv                                   # (the same point of the lattice, whichever image each side stores)
    assert np.abs(d).max() < 1e-8, np.abs(d).max()


@pytest.mark.parametrize("dtype,mesh,force_fft", [(np.float64, (600, 6, 7), False), (np.float32, (8, 520, 6), False), (np.float64, (21, 22, 25), True), (np.float32, None, True)])
def test_reciprocal_space_through_the_fft_library_vs_oracle(pkg, monkeypatch, dtype, mesh, force_fft):
    """Meshes with more than 512 points on an axis (the direct-DFT passes stop there) take hipFFT's real ↔ complex 3-D transforms with the influence function
    as a pass of its own (csrc/pme_fft.h, k_pme_conv; plan_fft! / plan_bfft!, ewald.jl:405-411).  Checked on long thin meshes the oracle's direct sums
    still finish on, and — forced with MOLLYHIP_PME_FFT=1 — on the meshes of the other tests."""
    if force_fft: monkeypatch.setenv("MOLLYHIP_PME_FFT", "1")
    else: monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    pme = dict(order=5, error_tol=5e-4)
    if mesh: pme["mesh"] = mesh
    case = S.charged_fluid(9, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=dtype, pme=pme, r_list=1.0, with_exceptions=False)
    o = case.oracle(np.float64)
    f_ref = o.forces(None, pairwise=False, specific=False, general=True, nthreads=8)
    e_ref = o.potential_energy(None, pairwise=False, general=True)
    s = case.system(pkg, dtype)
    f = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    assert s.stats()["pme_fft"] == 1                                          # the library ran: by the mesh's long axis, or because the switch (read at set-up) forces it
    e = pkg.potential_energy(s, pairwise=False, specific=False)
    w = pkg.virial(s, pairwise=False, specific=False)
    scale = np.linalg.norm(f_ref, axis=1).max()
    rel_f, rel_e = (1e-10, 1e-11) if dtype == np.float64 else (2e-4, 2e-5)
    assert np.linalg.norm(f - f_ref, axis=1).max() < rel_f * scale, np.linalg.norm(f - f_ref, axis=1).max() / scale
    assert abs(e - e_ref) < rel_e * abs(e_ref)
    w_ref = o.virial(None, pairwise=False, specific=False, general=True)
    assert np.abs(w - w_ref).max() < (1e-9 if dtype == np.float64 else 2e-4) * np.abs(w_ref).max()
    # a second call: the charge mesh was left zeroed
    f2 = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    assert np.linalg.norm(f2 - f_ref, axis=1).max() < rel_f * scale


def test_6mrr_in_a_triclinic_cell_without_tilt_vs_openmm(pkg):
    """the complete fp64 system (pair + bonded + Ewald exclusions + PME) declared as a TriclinicBoundary whose basis is the cubic box: every triclinic code
    path — cell grid in fractional coordinates, exact minimum image, recip_box — against the OpenMM fixture of the cubic system (test/protein.jl:267)"""
    d = G.data()
    case = G.case("ewald", np.float64, bonded=True, approx_erfc=False, pme=True)
    case.triclinic = dict(basis=np.diag(np.asarray(case.box, dtype=np.float64)), approx_images=False)
    s = case.system(pkg, np.float64)
    f = pkg.forces(s)
    assert np.linalg.norm(f - d["openmm_forces_all_pme_exact"], axis=1).max() < 1e-6
    e = pkg.potential_energy(s) + G.lj_dispersion_correction(d)
    assert abs(e - float(d["openmm_energy_all_pme_exact"])) < 1e-4


def test_6mrr_steps_through_the_fft_library_match_the_direct_passes(pkg, monkeypatch):
    """the complete fp32 MD step with the transforms in hipFFT (forced: 6mrr's mesh is 46 × 46 × 51; the switch is read at set-up and the stats say which path a context
    runs) against the default passes: 20 steps.  For scale: the oracle's own fp32 run is 3.5e-6 nm off its fp64 run over the same 20 steps (measured on the CPU)."""
    def run(fft):
        if fft: monkeypatch.setenv("MOLLYHIP_PME_FFT", "1")
        else: monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
        case = G.case("ewald", np.float32, bonded=True, pme=True)
        s = case.system(pkg, np.float32)
        pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 20)
        assert s.stats()["pme_fft"] == (1 if fft else 0)
        return np.array(s.coords, dtype=np.float64)
    x1, x0 = run(True), run(False)
    dlt = x1 - x0; dlt -= np.round(dlt / G.data()["box"]) * G.data()["box"]
    print(f"6mrr, library against direct passes after 20 steps: max |dx| {np.abs(dlt).max():.3e} nm")
    assert np.abs(dlt).max() < 5e-6
