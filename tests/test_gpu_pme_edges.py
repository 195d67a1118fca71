"""Reciprocal-space PME on the device (csrc/pme.h: spreading, the direct-DFT passes and the library transforms, interpolation; step_fused.h and forces_gs.hip: the
same jobs as parts of other launches) against the fp64 oracle on the same fp32-rounded inputs, per atom, at the edges of its loops: transform lengths between
257 and 512 (two rounds per line), at the steps of the lines-per-block count and at n = order; the three spreading paths, each forced and asserted
(tests/pme_ref.spread_paths on the engine's own atom order); atom counts that take the batch loops round a second time; every launch form of a step with charge on
every atom; and the state a call leaves behind.  The oracle itself is pinned to the exact Ewald sum in tests/test_pme_host.py.

Bars.  fp64: forces 1e-10 of the largest force per atom, energy 1e-11, virial 1e-9 of its largest component; run velocities 1e-9·V_i.  fp32 on meshes of at most
64 points per axis: 2e-4, 2e-5, 2e-4 (tests/test_gpu_pme.py).  fp32 on longer axes: those times sqrt(n_max/51) — they were set on 51-term sums, the oracle's float
instantiation transforms in double and is no yardstick for the length of a sum, and rounding grows like a random walk in the number of terms (3.2× at 512).  fp32
runs: twice the oracle's own fp32-against-fp64 figure (test_pme_host.YARD32_RUN).  Every fp32 ratio goes through the `slack` fixture.  Every case compares all of its
atoms (the error array has one finite entry per atom) and atoms without a charge must have exactly no force."""
import math

import numpy as np
import pytest

from tests import bonded_ref as B
from tests import pme_ref as R
from tests import systems as S
from tests.test_gpu_bonded import sorted_order
from tests.test_oracle_stochastic import KB
from tests.test_pme_host import LARGE_SIDE, RUN_STEPS, YARD32_RUN, charged_with_chains

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
FP64_BARS, FP32_BARS = (1e-10, 1e-11, 1e-9), (2e-4, 2e-5, 2e-4)


def bars(dtype, mesh):
    if dtype == np.float64:
        return FP64_BARS
    g = math.sqrt(max(mesh) / 51.0) if max(mesh) > 64 else 1.0
    return tuple(b * g for b in FP32_BARS)


_ref = {}


def reference(case):
    """fp64 oracle (forces, energy, virial) of a case: once per system, shared by its fp64 and fp32 runs and by both transform paths, never modified"""
    key = (case.name, case.n, tuple(case.pme_params(np.float64)["mesh"]), case.pme["order"], tuple(case.box))
    if key not in _ref:
        f, e, w = R.oracle_pme(case)
        f.setflags(write=False); w.setflags(write=False)
        _ref[key] = (f, e, w, case.coords.copy(), case.charge.copy())
    f, e, w, x, q = _ref[key]
    assert np.array_equal(x, case.coords) and np.array_equal(q, case.charge), "two different systems under one name"
    return f, e, w


def device(pkg, s):
    return (pkg.forces(s, pairwise=False, specific=False).astype(np.float64), pkg.potential_energy(s, pairwise=False, specific=False), pkg.virial(s, pairwise=False, specific=False))


def compare(case, dtype, got, slack, tag, mesh=None, force_scale=None):
    f_ref, e_ref, w_ref = reference(case)
    f, e, w = got
    bf, be, bw = bars(dtype, mesh or case.pme_params(dtype)["mesh"])
    assert f.shape == f_ref.shape == (case.n, 3) and np.isfinite(f).all() and math.isfinite(e) and np.isfinite(w).all()
    err = np.linalg.norm(f - f_ref, axis=1)
    assert err.shape == (case.n,)                                           # every atom is compared
    charged = case.charge != 0
    assert np.all(f[~charged] == 0.0), "an atom without a charge got a reciprocal-space force"
    assert np.all(np.linalg.norm(f_ref[charged], axis=1) > 0)
    rf, re, rw = float(err.max() / (force_scale or np.linalg.norm(f_ref, axis=1).max())), abs(e - e_ref) / abs(e_ref), float(np.abs(w - w_ref).max() / np.abs(w_ref).max())
    print(f"[pme edges] {tag} {np.dtype(dtype).name}: forces {rf:.3e} (bar {bf:.3e}, atom {int(err.argmax())})  energy {re:.3e} (bar {be:.3e})  virial {rw:.3e} (bar {bw:.3e})  atoms {case.n}")
    if dtype == np.float32:
        slack(f"{tag}: worst per-atom force error / largest force", rf, bf); slack(f"{tag}: energy, relative", re, be); slack(f"{tag}: virial / largest component", rw, bw)
    else:
        assert rf <= bf and re <= be and rw <= bw, (tag, (rf, re, rw), (bf, be, bw))


def check(pkg, case, dtype, slack, tag, fft=0, force_scale=None):
    s = case.system(pkg, dtype)
    got = device(pkg, s)
    assert s.stats()["pme_fft"] == fft
    compare(case, dtype, got, slack, tag, force_scale=force_scale)
    return s


def paths_of(pkg, s, case, dtype):
    """the spreading path of every batch of 64, from the engine's own atom order"""
    perm = sorted_order(pkg, s, case.n)
    assert np.array_equal(np.sort(perm), np.arange(case.n))
    p = case.pme_params(dtype)
    return R.spread_paths(case.coords[perm].astype(dtype), case.charge[perm], p["mesh"], p["order"], case.box), perm


# ---- 1. transform lengths ---------------------------------------------------------------------------------------------
LONG = [(257, 6, 6), (300, 6, 7), (384, 7, 8), (512, 9, 6), (6, 257, 8), (7, 300, 6), (6, 384, 8), (8, 512, 7), (6, 7, 257), (9, 6, 300), (6, 8, 384), (8, 6, 512)]
STEPS = [(128, 6, 7), (129, 7, 6), (256, 6, 8), (6, 7, 128), (7, 6, 129), (6, 8, 256)]      # lines per block 2 → 1 (x, y), 3 → 1 (real-to-complex) and 2 → 1 (complex-to-real)


def fluid7(mesh, order=5, box_scale=(1.0, 1.0, 1.0)):
    c = S.charged_fluid(7, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=np.float32, pme=dict(order=order, mesh=mesh), r_list=1.0, with_exceptions=False, box_scale=box_scale)
    c.name = f"fluid7_{box_scale}"
    return c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh", LONG + STEPS, ids=lambda m: "x".join(map(str, m)))
def test_direct_passes_at_every_line_length(pkg, monkeypatch, slack, mesh, dtype):
    """343 charges (box 2.17 nm), one axis of 257 … 512 points — two rounds of every `o += 256` loop of the three pass bodies, the second sweep of the x pass over its
    products included; along z: 257 half-spectrum outputs and 512 real outputs per line, odd and even lengths — and of 128, 129, 256, where the number of lines a
    block stages steps down.  The fp64 run at 1e-10 is what proves the index arithmetic."""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    assert max(mesh) <= 512 and (max(mesh) > 256) == (mesh in LONG)
    check(pkg, fluid7(mesh), dtype, slack, "direct " + "x".join(map(str, mesh)), fft=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh", LONG, ids=lambda m: "x".join(map(str, m)))
def test_long_meshes_through_the_fft_library(pkg, monkeypatch, slack, mesh, dtype):
    """the same meshes with the transforms in the library and the influence function as a pass of its own (k_pme_conv), against the same reference"""
    monkeypatch.setenv("MOLLYHIP_PME_FFT", "1")
    check(pkg, fluid7(mesh), dtype, slack, "library " + "x".join(map(str, mesh)), fft=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [4, 5, 6])
def test_smallest_legal_mesh(pkg, monkeypatch, slack, order, dtype):
    """n = order on every axis: each atom's weights cover every mesh point of an axis exactly once, every index wraps"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    check(pkg, fluid7((order,) * 3, order), dtype, slack, f"n = order = {order}", fft=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_even_orthorhombic_mesh_in_the_direct_path(pkg, monkeypatch, slack, dtype):
    """mesh (24, 22, 26) on a box of three different sides: Nyquist planes on all three axes in the non-triclinic branch of the influence function — the virial's
    mixed components of a Nyquist axis and a regular one cancel between k and −k there"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    case = fluid7((24, 22, 26), box_scale=(1.0, 1.1, 1.2))
    assert len(set(case.box)) == 3
    check(pkg, case, dtype, slack, "all-even 24x22x26", fft=0)


# ---- 2. spreading and gather edges -----------------------------------------------------------------------------------
BOX, MESH32 = 2.4, (32, 32, 32)          # spacing 0.075 nm


def cluster(rng, centre, m, spacings=3.0, sp=BOX / 32):
    return (np.asarray(centre) + rng.uniform(0, spacings * sp, (m, 3))) % BOX


def neutral(rng, m):
    q = rng.uniform(0.2, 1.0, m) * rng.choice([-1.0, 1.0], m)
    return q - q.mean()


def run_paths(pkg, case, dtype, slack, tag, want, force_scale=None):
    s = check(pkg, case, dtype, slack, tag, force_scale=force_scale)
    got, perm = paths_of(pkg, s, case, dtype)
    print(f"[pme edges] {tag}: paths {got}")
    assert got == want if isinstance(want, list) else want(got), (tag, got)
    return s, perm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 129])
def test_atom_counts_at_batch_edges(pkg, monkeypatch, slack, n, dtype):
    """n random charges (orders 4, 5, 6 in turn): one short of, at and one over the gather's batch of 16 and the spreading's batch of 64, a single atom (a net
    charge), two.  A single atom and a pair fit the sub-mesh; batches of atoms all over the box do not.
    The exact force on a single charge in a periodic cell is zero by symmetry: what the oracle has there is the self-force residue of the discretisation, the sum of
    the atom's own mesh terms cancelling to a part in 10⁴ — no scale for an error.  The single atom's force is measured against ke·q²/L², the force between the charge
    and its nearest image (the terms that cancel are larger: ke·q²·α²)."""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    order = 4 + n % 3
    case = R.random_charges(n, BOX, order, (32, 30, 36), net=0.5 if n == 1 else 0.0)
    want = (lambda g: g == ["lds"]) if n == 1 else (lambda g: len(g) == -(-n // 64) and "empty" not in g)
    run_paths(pkg, case, dtype, slack, f"{n} atoms, order {order}", want, force_scale=R.KE * case.charge[0] ** 2 / case.box.min() ** 2 if n == 1 else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [4, 5, 6])
@pytest.mark.parametrize("where", ["inside", "corner"])
def test_compact_batches_take_the_lds_sub_mesh(pkg, monkeypatch, slack, where, order, dtype):
    """70 charges inside a cube of 3 mesh spacings: both batches fit the sub-mesh; in the box corner the sub-mesh wraps all three periodic boundaries in its flush"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    rng = np.random.default_rng(11)
    sp = BOX / 32
    x = cluster(rng, [1.0, 1.3, 0.7] if where == "inside" else [-1.5 * sp] * 3, 70)
    case = R.point_charges(x, neutral(rng, 70), BOX, order, MESH32, name=f"cluster_{where}")
    idx, _ = R.place(case.coords.astype(dtype), MESH32, case.box)
    if where == "corner":
        assert all({0, 31} <= set(idx[:, d]) for d in range(3))
    run_paths(pkg, case, dtype, slack, f"cluster {where}, order {order}", ["lds", "lds"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [4, 6])
def test_batches_all_over_the_box_take_the_direct_path(pkg, monkeypatch, slack, order, dtype):
    """256 charges uniform over the box on a 32³ mesh: every batch's extents exceed the mesh"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    run_paths(pkg, R.random_charges(256, BOX, order, MESH32, seed=3), dtype, slack, f"uniform 256, order {order}", ["direct"] * 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_batch_of_more_cells_than_the_sub_mesh_takes_the_direct_path(pkg, monkeypatch, slack, dtype):
    """mesh 96³: 64 charges in a cube of 20 spacings — extents of about 25 fit the mesh, 25³ cells do not fit the 6144 of the sub-mesh; beside it a batch in a cube of
    8 spacings that does (at most 14³ = 2744)"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    rng = np.random.default_rng(12)
    sp = BOX / 96
    x = np.concatenate([cluster(rng, [0.4, 0.5, 0.6], 64, 20.0, sp), cluster(rng, [1.5, 1.5, 1.5], 64, 8.0, sp)])
    case = R.point_charges(x, np.concatenate([neutral(rng, 64), neutral(rng, 64)]), BOX, 5, (96,) * 3, name="wide_batch")
    assert R.spread_paths(case.coords.astype(dtype), case.charge, (96,) * 3, 5, case.box, cells=10 ** 9) == ["lds", "lds"]      # (only the cell count stands in the way)
    run_paths(pkg, case, dtype, slack, "wide batch on 96^3", ["direct", "lds"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_charges(pkg, monkeypatch, slack, dtype):
    """whole batches without a charge (skipped), a compact charged batch between them, a single charged atom at the end of a batch of zero charges (its box is that atom
    alone, wherever the others sit), and a last short batch: the atoms without a charge have exactly no force (asserted in compare)"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    rng = np.random.default_rng(13)
    x = np.concatenate([rng.uniform(0, BOX, (64, 3)), cluster(rng, [0.8, 1.9, 0.3], 64), rng.uniform(0, BOX, (64, 3)), rng.uniform(0, BOX, (64, 3)), rng.uniform(0, BOX, (5, 3))])
    q = np.zeros(len(x))
    q[64:128] = neutral(rng, 64); q[64] += 0.375
    q[255] = -0.25; q[258] = -0.125
    case = R.point_charges(x, q, BOX, 5, MESH32, name="zeros")
    assert abs(case.charge.sum()) < 1e-6 and (case.charge == 0).sum() == 195
    run_paths(pkg, case, dtype, slack, "zero charges", ["empty", "lds", "empty", "lds", "lds"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [4, 5, 6])
def test_atoms_on_mesh_nodes_and_on_the_faces_of_the_box(pkg, monkeypatch, slack, order, dtype):
    """box 2.0 nm, mesh 32³ (1/L, the spacing of 1/16 nm and the nodes are exact in both precisions, so the offsets are exactly 0): every atom on a mesh node (offset 0: the last weight vanishes) — coordinate 0, nodes on either
    side of the faces — or at the largest number below the box length, axis by axis.  Round the corner the batch is compact: the sub-mesh."""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    L = 2.0
    top = float(np.nextafter(dtype(L), dtype(0)))
    vals = [0.0, 0.0625, 0.125, L - 0.0625, L - 0.125, top]
    rng = np.random.default_rng(14)
    x = rng.choice(vals, (36, 3))
    x[0] = 0.0; x[1] = top
    case = R.point_charges(x, neutral(rng, 36), L, order, MESH32, dtype=dtype, name=f"nodes_{np.dtype(dtype).name}")
    assert np.array_equal(case.coords, x) and (case.coords == top).any(axis=0).all() and (case.coords == 0).any(axis=0).all()
    run_paths(pkg, case, dtype, slack, f"nodes and faces, order {order}", ["lds"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beyond", [False, True])
def test_charges_at_the_edge_of_the_fixed_point_range(pkg, monkeypatch, slack, beyond, dtype):
    """order 4, q = ±24 on mesh nodes: the largest term the fixed-point sub-mesh is ever handed, q·w·2²⁸ = 24·(2/3)³·2²⁸ = 1.91e9 < 2³¹ in fp32 — and the next number above
    24, which sends the batch down the direct path.  40 atoms in a cube of 3 spacings, neutral."""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    rng = np.random.default_rng(15)
    x = cluster(rng, [1.0, 1.0, 1.0], 40, sp=0.0625)
    x[3] = [1.0625, 1.125, 1.0]; x[17] = [1.125, 1.0625, 1.0625]           # mesh nodes of a 32³ mesh on 2.0 nm (1/L exact: the offsets are exactly 0)
    q = neutral(rng, 40)
    rest = np.ones(40, bool); rest[[3, 17]] = False
    q[rest] -= q[rest].mean()                                                # the other 38 are neutral among themselves
    big = float(np.nextafter(dtype(24), dtype(np.inf))) if beyond else 24.0
    q[3], q[17] = big, -big
    case = R.point_charges(x, q, 2.0, 4, MESH32, dtype=dtype, name=f"q24_{beyond}_{np.dtype(dtype).name}")
    idx, dr = R.place(case.coords[[3, 17]].astype(dtype), MESH32, case.box)
    assert np.all(dr == 0) and abs(case.charge.sum()) < 1e-5 and np.abs(case.charge).max() == big
    assert 24 * (2 / 3) ** 3 * 2 ** 28 < 2 ** 31 - 1
    run_paths(pkg, case, dtype, slack, f"|q| = {big!r}", ["direct" if beyond else "lds"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_charges_on_the_fixed_point_sub_mesh(pkg, monkeypatch, slack, dtype):
    """the charges of charged_fluid(8) times 2⁻⁸, in the engine's sorted order (a pair pass first: compact batches, the sub-mesh).  The physics is scale-free, so the
    bars are the unscaled ones; the 2⁻²⁸ rounding of the fp32 sub-mesh has a share of 4.6e-6 of the largest force at this scale (emulated in the CPU oracle)."""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    case = S.charged_fluid(8, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=np.float32, pme=dict(order=5, error_tol=5e-4), r_list=1.0, with_exceptions=False)
    case.charge = case.charge * 2.0 ** -8
    case.name = "charged512_small_q"
    s = case.system(pkg, dtype)
    pkg.forces(s)                                                           # the pair pass sorts the atoms
    compare(case, dtype, device(pkg, s), slack, "charges x 2^-8")
    got, perm = paths_of(pkg, s, case, dtype)
    assert not np.array_equal(perm, np.arange(case.n)) and got.count("lds") >= 6 and "empty" not in got, got


@pytest.mark.parametrize("dtype", DTYPES)
def test_net_charge(pkg, monkeypatch, slack, dtype):
    """65 charges summing to +3 e: the net-charge term of the energy and on the diagonal of the virial"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    case = R.random_charges(65, (2.2, 2.35, 2.5), 5, (30, 32, 34), net=3.0, name="net3")
    term = R.KE * np.pi * case.charge.sum() ** 2 / (2 * np.prod(case.box) * R.alpha_of(case) ** 2)
    f_ref, e_ref, w_ref = reference(case)
    assert abs(case.charge.sum() - 3.0) < 1e-5 and term > 10 * FP32_BARS[1] * abs(e_ref) and term > 10 * FP32_BARS[2] * np.abs(w_ref).max()      # (left out, it would show)
    check(pkg, case, dtype, slack, "net charge +3")


# ---- 3. the batch loops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_side,mesh", [(33, (40, 36, 45)), (52, (48, 40, 54))])
def test_second_trip_of_the_batch_loops(pkg, monkeypatch, slack, n_side, mesh, dtype):
    """35 937 atoms: more than 2048 gather batches of 16; 140 608 atoms: more than 2048 spreading batches of 64.  Per atom: a batch that was skipped or done twice is an
    error of the size of a typical force."""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    case = S.charged_fluid(n_side, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=np.float32, pme=dict(order=5, mesh=mesh), r_list=1.0, with_exceptions=False)
    case.name = f"fluid{n_side}"
    assert case.n > 2048 * (16 if n_side == 33 else 64) and case.n <= 2 * 2048 * 64
    check(pkg, case, dtype, slack, f"{case.n} atoms")


# ---- 4. launch forms with charge everywhere ----------------------------------------------------------------------------
FORMS = {   # dtype, MOLLYHIP_GROUP_SPLIT, MOLLYHIP_FUSE_GATHER_VV
    "group_split_integrating": (np.float32, None, "1"),
    "group_split_collect": (np.float32, None, "0"),
    "spread_bonded_integrating": (np.float32, "0", "1"),
    "spread_bonded_collect": (np.float32, "0", "0"),
    "fp64_integrating": (np.float64, "0", "1"),
    "fp64_collect": (np.float64, "0", "0"),
}
_run_ref = {}


def run_reference(case):
    if case.name not in _run_ref:
        v, sc = B.oracle_run(case, np.float64, RUN_STEPS), B.velocity_scale(case, RUN_STEPS)
        v.setflags(write=False); sc.setflags(write=False)
        _run_ref[case.name] = (v, sc)
    return _run_ref[case.name]


def check_run(pkg, monkeypatch, slack, case, dtype, split, fuse, yard, tag, want_split):
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    if split is None: monkeypatch.delenv("MOLLYHIP_GROUP_SPLIT", raising=False)
    else: monkeypatch.setenv("MOLLYHIP_GROUP_SPLIT", split)
    monkeypatch.setenv("MOLLYHIP_FUSE_GATHER_VV", fuse)
    s = case.system(pkg, dtype)
    pkg.simulate(s, pkg.VelocityVerlet(dt=B.RUN_DT), RUN_STEPS)
    st = s.stats()
    print(f"[pme edges] run {tag}: group_split {st['group_split']}, group-split passes {st['n_group_split_passes']}, integrating launches {st['n_fused_steps']}")
    assert (st["n_group_split_passes"] > 0) == want_split and (st["n_fused_steps"] > 0) == (fuse == "1"), st
    v_ref, scale = run_reference(case)
    assert scale.shape == (case.n,) and np.all(scale > 0)                   # every atom is compared
    r = np.linalg.norm(np.asarray(s.velocities, dtype=np.float64) - v_ref, axis=1) / scale
    assert np.isfinite(r).all()
    print(f"[pme edges] run {tag}: worst ‖Δv_i‖/V_i {r.max():.3e} (atom {int(r.argmax())})")
    if dtype == np.float32:
        slack(f"run {tag}: worst ‖Δv_i‖/V_i", r.max(), 2.0 * yard)
    else:
        assert r.max() <= 1e-9, r.max()


@pytest.mark.parametrize("order", [4, 5, 6])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_launch_forms_of_a_step_with_charge_on_every_atom(pkg, monkeypatch, slack, form, order):
    """the charged fluid with chains (test_pme_host.charged_with_chains: about 1 950 atoms, all charged, bonded terms present), at rest, RUN_STEPS velocity-Verlet steps:
    spreading inside the group-split pair launch (its dynamic-LDS sub-mesh), k_spread_bonded, k_gather_collect and the integrating k_gather_collect_vv, orders 4–6,
    in fp32 and (without the group split) fp64.  Velocities per atom against the fp64 oracle's run."""
    dtype, split, fuse = FORMS[form]
    check_run(pkg, monkeypatch, slack, charged_with_chains(order), dtype, split, fuse, YARD32_RUN[f"small_o{order}"], f"{form} order {order}", want_split=split is None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_integrating_launch_takes_a_second_batch(pkg, monkeypatch, slack, dtype):
    """about 36 000 atoms: too many for the group split (k_spread_bonded spreads), and more than 2048 batches of 16 in the integrating launch — its second trip, with
    the barrier that exists for it alone"""
    case = charged_with_chains(5, n_side=LARGE_SIDE)
    assert case.n > 2048 * 16
    check_run(pkg, monkeypatch, slack, case, dtype, None, "1", YARD32_RUN["large_o5"], f"{case.n} atoms", want_split=False)


def test_langevin_inside_the_integrating_launch_on_a_small_system_fp64(pkg, monkeypatch):
    """k_gather_collect_vv's Langevin instantiation away from 6mrr: in fp64 the device's noise is the oracle's, 8 steps at the fp64 trajectory bars of
    tests/test_gpu_stochastic.py"""
    monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False); monkeypatch.delenv("MOLLYHIP_GROUP_SPLIT", raising=False)
    monkeypatch.setenv("MOLLYHIP_FUSE_GATHER_VV", "1")
    case = charged_with_chains(5)
    rng = np.random.default_rng(6)
    key, ctr1 = (int(rng.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(2))
    o = case.oracle(np.float64)
    o.langevin_run(8, 0.0005, KB * 300.0, 1.0, key=key, ctr1=ctr1, remove_cm_every=1, nthreads=4, specific=True, general=True)
    s = case.system(pkg, np.float64)
    pkg.simulate(s, pkg.Langevin(dt=0.0005, temperature=300.0, friction=1.0), 8, rng=6)
    d = s.coords - o.coords
    d -= np.round(d / case.box) * case.box
    print("[pme edges] langevin fp64: max |dx|", np.abs(d).max(), "max |dv|", np.abs(s.velocities - o.vel).max())
    assert d.shape == (case.n, 3) and np.abs(d).max() < 1e-9 and np.abs(s.velocities - o.vel).max() < 1e-6
    assert s.stats()["n_fused_steps"] >= 7


# ---- 5. the mesh is left clean ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fft", [0, 1])
def test_every_call_leaves_the_meshes_as_it_found_them(pkg, monkeypatch, slack, fft, dtype):
    """energy only (no backward transform, no interpolation), forces, virial, three steps of a run, forces again on one context: each result is what a fresh context
    gives for the same coordinates — nothing of a call is left on the charge mesh or in the half spectrum, through the direct passes and through the library"""
    if fft: monkeypatch.setenv("MOLLYHIP_PME_FFT", "1")
    else: monkeypatch.delenv("MOLLYHIP_PME_FFT", raising=False)
    case = S.charged_fluid(8, dict(kind="ewald", rc=0.9, tol=5e-4), dtype=np.float32, pme=dict(order=5, mesh=(24, 25, 26)), r_list=1.0, with_exceptions=False, stable=True)
    case.name = "clean512"
    f_ref, e_ref, w_ref = reference(case)
    s = case.system(pkg, dtype)
    e = pkg.potential_energy(s, pairwise=False, specific=False)
    f = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    w = pkg.virial(s, pairwise=False, specific=False)
    assert s.stats()["pme_fft"] == fft
    compare(case, dtype, (f, e, w), slack, f"sequence, fft {fft}")
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.0005), 3)
    moved = S.Case(np.asarray(s.coords, dtype=np.float64), case.box, coul=case.coul, r_list=case.r_list, charge=case.charge, mass=case.mass, velocities=np.zeros((case.n, 3)),
                   pme=case.pme, name=f"clean512_moved_{fft}_{np.dtype(dtype).name}")
    assert np.abs(moved.coords - case.coords).max() > 1e-5
    compare(moved, dtype, device(pkg, s), slack, f"after 3 steps, fft {fft}")
    fresh = moved.system(pkg, dtype)
    f2 = pkg.forces(fresh, pairwise=False, specific=False).astype(np.float64)
    f1 = pkg.forces(s, pairwise=False, specific=False).astype(np.float64)
    bf = bars(dtype, (24, 25, 26))[0]
    assert np.linalg.norm(f1 - f2, axis=1).max() <= bf * np.linalg.norm(f_ref, axis=1).max()
