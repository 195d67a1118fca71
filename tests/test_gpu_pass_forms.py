"""Which form the plain pass of an fp32 one-type fluid takes follows from the largest tile of its inner list (csrc/pass_plan.h): the packed loop with
the tile as x[] / y[] / z[] of 2049, 3073 or 4097 dwords while tile + 1 is below the stride — the only pass that integrates in its epilogue — and the
generic loop from 4096 atoms on.  One dense fluid, four list radii, one per band; every case confirms from mhip_get_stats what ran.

The system: 27 000 atoms on a jittered lattice of 0.3 nm (σ = 0.282 nm: argon's σ / spacing), box 9 nm, 256 x 2 blocks, cutoff r_list − 0.1 nm so that the
inner list is pruned to r_list itself.  mhip_get_stats has no figure for the inner list's largest tile (max_tile_atoms is the outer list's), so the band
is read from lds_bytes: 12·stride + 64 names the stride, and the generic loop's (tile + 1)·16 + 32 the tile itself.  Seen on an MI355X:

    r_list   max_tile_atoms (outer list)   lds_bytes of the plain pass   inner tile
    0.8      2191                          24 652 (stride 2049)          below 2048
    1.15     3684                          36 940 (stride 3073)          2048 … 3071
    1.5      4988                          49 228 (stride 4097)          3072 … 4095
    1.6      5703                          69 168 (generic)              4320

and 19 of the 20 steps integrate in the pass in the first three rows (step 0 prunes), none in the fourth.  The neighbours of these radii that were
tried: 1.7 nm is served in 128 x 4 blocks with the in-loop minimum image (the outer tile of a 256-atom block no longer fits the search).
"""
import math

import numpy as np
import pytest

from tests import systems as S

pytestmark = pytest.mark.gpu

SPACING, N_SIDE, SKIN = 0.3, 30, 0.1
STRIDES = (2049, 3073, 4097)
BANDS = {"below_2048": (0.8, 0), "2048_to_3071": (1.15, 1), "3072_to_4095": (1.5, 2), "4096_and_above": (1.6, 3)}      # r_list, band


def dense_fluid(r_list):
    n = N_SIDE ** 3
    g = np.stack(np.meshgrid(*[np.arange(N_SIDE)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    box = float(np.float32(N_SIDE * SPACING))
    x = (g + 0.5) * SPACING + np.random.default_rng(2).uniform(-0.05 * SPACING, 0.05 * SPACING, (n, 3))
    x = (x - np.floor(x / box) * box).astype(np.float32).astype(np.float64)
    x = np.where(x >= box, 0.0, x)
    v = np.random.default_rng(3).normal(size=(n, 3)) * math.sqrt(8.314462618e-3 * 85.0 / S.ARGON["mass"])
    v = (v - v.mean(axis=0)).astype(np.float32).astype(np.float64)
    return S.Case(x, box, lj=dict(cutoff=("distance", r_list - SKIN)), r_list=r_list, rebuild_every=10, velocities=v,
                  sigma=np.full(n, S.ARGON["sigma"] * SPACING / S.LJ_SPACING), eps=np.full(n, S.ARGON["eps"]), mass=np.full(n, S.ARGON["mass"]), name=f"dense{n}")


@pytest.mark.parametrize("band_name", list(BANDS))
def test_plain_pass_form_follows_the_inner_tile(pkg, band_name):
    r_list, band = BANDS[band_name]
    case = dense_fluid(r_list)
    s = case.system(pkg, np.float32)
    pkg.set_launch_config(s, 256, 2)
    pkg.simulate(s, pkg.VelocityVerlet(dt=0.002), 20)                  # mhip_vv_run: step 0 prunes, the others walk the inner list
    st = s.stats()                                                     # … whose form these figures show
    lds, outer, fused = st["lds_bytes"], st["max_tile_atoms"], st["n_fused_steps"]
    print(f"[pass forms] r_list {r_list}: max_tile_atoms {outer}, lds_bytes {lds}, tile_segments {st['tile_segments']}, fused steps {fused} of 20, prunes {st['n_filter_passes']}, searches {st['n_outer_builds']}")
    f = pkg.forces(s, step_n=21).astype(np.float64)                    # off the list cadence: the same lists, the same plain pass, now with the forces written out
    st1 = s.stats()
    if st1["n_filter_passes"] == st["n_filter_passes"] and st1["n_outer_builds"] == st["n_outer_builds"]:
        assert (st1["lds_bytes"], st1["tile_segments"]) == (lds, 1), (st1, st)
    assert (st["block_atoms"], st["j_split"], st["minimg_mode"], st["tile_segments"]) == (256, 2, 0, 1), st
    assert st["n_filter_passes"] >= 1 and st["n_group_split_passes"] == 0, st
    if band < 3:
        assert lds == 12 * STRIDES[band] + 64, (lds, [12 * q + 64 for q in STRIDES])      # the smallest stride above tile + 1: the inner tile lies in this band
        assert outer + 1 >= (STRIDES[band - 1] if band else 0)                             # (the outer list's tile is no smaller than the inner one's)
        assert fused > 0
    else:
        tile = (lds - 32) // 16 - 1                                                        # the generic loop: (tile + 1) float4 records + 32
        assert (lds - 32) % 16 == 0 and 4096 <= tile <= outer, (lds, tile, outer)
        assert fused == 0
    tol, o, nl = S.fp32_force_tolerance(case, coords=np.asarray(s.coords, dtype=np.float64))
    S.fp32_check(np.linalg.norm(f - o.forces(nl), axis=1), tol, f"forces of the plain pass, inner tile band {band_name}")
