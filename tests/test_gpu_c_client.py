"""The C ABI driven by C programs (tests/c_client/mhip_drive.c and mhip_drive_topology.c, gcc, no Python in the call path): create → set_atoms → set_state →
forces / energies → vv_run → get_state → set_state + forces(step_n) × 5 → stats → set_box (a trial move and back) → destroy.  Its numbers are checked against the CPU
oracle on the same inputs: fp64 forces and energies at the reference's bars (test/protein.jl:267, 274), the 20-step trajectory at
1e-9 nm, and the drop-in cadence (no new neighbour search for unchanged coordinates).  The second program makes the set-up calls of the Julia shim for a
protein (exceptions, bonded terms, Ewald exclusions, PME) and the neighbour export, CM removal, random velocities and Langevin run after them."""
import os
import subprocess

import numpy as np
import pytest

from tests import systems as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_client_drives_the_engine(tmp_path):
    exe, out = tmp_path / "mhip_drive", tmp_path / "out.bin"
    lib_dir = os.path.join(ROOT, "molly.jl_amd")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_client", "mhip_drive.c"),
                    "-o", str(exe), "-L", lib_dir, "-l:libmollyhip.so", f"-Wl,-rpath,{lib_dir}", "-Wl,--allow-shlib-undefined", "-lm"], check=True)
    n_side, n_steps = 12, 20
    r = subprocess.run([str(exe), str(n_side), str(n_steps), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = np.fromfile(out, dtype=np.float64)
    n = int(raw[0]); box, dt = raw[1], raw[2]
    pe0, ke0, pe1, ke1 = raw[4:8]
    body = raw[8:8 + 18 * n].reshape(6, n, 3)
    x0, v0, f0, x1, v1, f1 = body
    searches, prunes, calls, pairs_full, pe_scaled, pe_back = raw[8 + 18 * n:]
    assert n == n_side ** 3 and int(raw[3]) == n_steps
    case = S.Case(x0, box, lj=dict(cutoff=("distance", 1.0)), r_list=1.2, rebuild_every=10, velocities=v0,
                  sigma=np.full(n, 0.34), eps=np.full(n, 0.997), mass=np.full(n, 39.948))
    o = case.oracle(np.float64)
    nl = o.neighbors("cell")
    f_ref = o.forces(nl)
    assert np.abs(f0 - f_ref).max() < 1e-7                                   # kJ/mol/nm, test/protein.jl:267
    assert pe0 == pytest.approx(o.potential_energy(nl), rel=1e-10, abs=1e-6)         # the reference's bar is 1e-5 kJ/mol on ~1e5 (protein.jl:274)
    assert ke0 == pytest.approx(o.kinetic_energy(), rel=1e-12)
    o.vv_run(n_steps, dt, remove_cm_every=1)
    d = x1 - o.coords
    d -= np.round(d / box) * box
    assert np.abs(d).max() < 1e-9 and np.abs(v1 - o.vel).max() < 1e-8
    assert ke1 == pytest.approx(o.kinetic_energy(), rel=1e-9)
    # the set_state → forces(step_n) loop on unchanged coordinates: correct forces, and no search was needed for them
    o2 = case.oracle(np.float64, coords=x1)
    nl2 = o2.neighbors("cell")
    f1_ref = o2.forces(nl2)
    assert int(pairs_full) == 2 * len(nl2[0])                                # the statistics count the reference's list of the final coordinates
    assert np.abs(f1 - f1_ref).max() < 1e-7
    assert int(calls) == 5 and int(searches) == 0 and int(prunes) <= 1
    # mhip_set_box: the energy on the box scaled by 1 % (coordinates with it), and the old energy after the move is taken back
    o3 = S.Case(1.01 * x1, 1.01 * box, lj=dict(cutoff=("distance", 1.0)), r_list=1.2, rebuild_every=10, sigma=np.full(n, 0.34), eps=np.full(n, 0.997),
                mass=np.full(n, 39.948)).oracle(np.float64)
    assert pe_scaled == pytest.approx(o3.potential_energy(o3.neighbors("cell")), rel=1e-10, abs=1e-6)
    assert pe_back == pytest.approx(pe1, rel=1e-11)


def _topology_input(pkg, case, path, rv, lang):
    """the input file of tests/c_client/mhip_drive_topology.c (layout in its header comment): the System's own arrays, as the shim hands them over"""
    from molly_jl_amd import _lib
    import ctypes as C
    s = case.system(pkg, np.float64)
    nf, gi = s.neighbor_finder, s.general_inters[0]
    cfg = _lib.Config()                                        # what System.engine() fills in (api.py)
    cfg.precision, cfg.device_id, cfg.n_atoms = 64, 0, len(s)
    for d in range(3):
        cfg.box[d] = s.boundary.side_lengths[d]; cfg.periodic[d] = 1
    cfg.rebuild_every, cfg.r_list, cfg.inter = nf.n_steps, nf.dist_cutoff, s.interactions()
    sil = {type(x).__name__: x for x in s.specific_inter_lists}
    b, a, t, w = sil["HarmonicBonds"], sil["HarmonicAngles"], sil["PeriodicTorsions"], sil["EwaldExclusions"]
    hdr = np.zeros(20, np.uint64)
    for k, val in enumerate([C.sizeof(cfg), len(s), len(nf.excluded), len(nf.special), len(b.i), len(a.i), len(t.i), len(w.i), gi.order, *gi.mesh_dims,
                             lang["n_steps"], rv["key"], rv["ctr1"], lang["key"], lang["ctr1"]]):
        hdr[k] = np.uint64(val)
    dh = np.zeros(8)
    dh[:6] = [gi.α, gi.ϵr, rv["kT"], lang["dt"], lang["kT"], lang["friction"]]
    i32 = lambda *xs: [np.ascontiguousarray(x, dtype=np.int32) for x in xs]
    f64 = lambda *xs: [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    parts = [hdr, dh, np.frombuffer(C.string_at(C.addressof(cfg), C.sizeof(cfg)), np.uint8),
             *f64(s.coords, s.velocities, s.charge, s.σ, s.ϵ, s.masses), *i32(nf.excluded[:, 0], nf.excluded[:, 1], nf.special[:, 0], nf.special[:, 1]),
             *i32(b.i, b.j), *f64(b.k, b.r0), *i32(a.i, a.j, a.k), *f64(a.kθ, a.θ0), *i32(t.i, t.j, t.k, t.l, t.periodicity), *f64(t.phase, t.k0),
             *i32(w.i, w.j)]
    with open(path, "wb") as fh:
        for p in parts:
            fh.write(np.ascontiguousarray(p).tobytes())


def test_c_client_makes_the_shims_topology_calls(pkg, tmp_path):
    """The set-up calls the shim makes for a real protein (exceptions, bonded terms, Ewald exclusions, PME), the neighbour export, the force parts
    accumulated into one buffer, the three energies, CM removal, random velocities and a Langevin run — from C, on 6mrr (Ewald with exact erfc + bonded
    + PME, fp64).  The pair set against the oracle's, forces and energy against OpenMM at test_all_pme_vs_openmm_fp64's bars, the velocities against
    the oracle with the same Philox words, the Langevin end state at test_langevin_fp64_6mrr_pme_matches_oracle's bars."""
    from tests import golden6mrr as G
    from tests.test_gpu_stochastic import draws
    from tests.test_oracle_stochastic import KB
    exe, inp, out = tmp_path / "mhip_drive_topology", tmp_path / "in.bin", tmp_path / "out.bin"
    lib_dir = os.path.join(ROOT, "molly.jl_amd")
    cc = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_client", "mhip_drive_topology.c"),
                         "-o", str(exe), "-L", lib_dir, "-l:libmollyhip.so", f"-Wl,-rpath,{lib_dir}", "-Wl,--allow-shlib-undefined", "-lm"], capture_output=True, text=True)
    assert cc.returncode == 0 and "warning" not in cc.stderr, cc.stderr
    case = G.case("ewald", np.float64, bonded=True, approx_erfc=False, pme=True)
    n = case.n
    ctr1_rv, key_rv = draws(31, 2)
    key_l, ctr1_l = draws(32, 2)
    rv = dict(kT=KB * 300.0, key=key_rv, ctr1=ctr1_rv)
    lang = dict(n_steps=10, dt=0.0005, kT=KB * 300.0, friction=1.0, key=key_l, ctr1=ctr1_l)
    _topology_input(pkg, case, inp, rv, lang)
    r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout

    raw = out.read_bytes()
    n_pairs = int(np.frombuffer(raw, np.int64, 1)[0]); off = 8
    pi = np.frombuffer(raw, np.int32, n_pairs, off); off += 4 * n_pairs
    pj = np.frombuffer(raw, np.int32, n_pairs, off); off += 4 * n_pairs
    psp = np.frombuffer(raw, np.uint8, n_pairs, off); off += n_pairs
    rest = np.frombuffer(raw, np.float64, offset=off)
    assert rest.size == 15 * n + 3
    f = rest[:3 * n].reshape(n, 3); pe = rest[3 * n:3 * n + 3]
    v_cm, v_rand, x_end, v_end = rest[3 * n + 3:].reshape(4, n, 3)

    o = case.oracle(np.float64)
    oi, oj, osp = o.neighbors("cell", nthreads=8)
    a, b = S.sorted_pairs(oi, oj, osp), S.sorted_pairs(pi, pj, psp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert n_pairs == 4602420 and int(psp.sum()) == 3094                                  # test_gpu_6mrr.py, test/basic.jl:592-593
    d = G.data()
    assert np.linalg.norm(f - d["openmm_forces_all_pme_exact"], axis=1).max() < 1e-6
    assert abs(pe.sum() + G.lj_dispersion_correction(d) - float(d["openmm_energy_all_pme_exact"])) < 1e-4
    o.remove_cm()
    assert np.abs(v_cm - o.vel).max() < 1e-12
    o.random_velocities(rv["kT"], key=key_rv, ctr1=ctr1_rv)
    assert np.abs(v_rand - o.vel).max() < 6e-13 * np.sqrt(rv["kT"] / case.mass.min())     # test_random_velocities_and_andersen_match_the_oracle
    ol = case.oracle(np.float64, velocities=v_rand)
    ol.langevin_run(lang["n_steps"], lang["dt"], lang["kT"], lang["friction"], key=key_l, ctr1=ctr1_l, remove_cm_every=1, nthreads=8, specific=True, general=True)
    dx = x_end - ol.coords
    dx -= np.round(dx / case.box) * case.box
    assert np.abs(dx).max() < 1e-9 and np.abs(v_end - ol.vel).max() < 1e-6
