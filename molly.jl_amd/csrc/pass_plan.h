// pass_plan.h — which pair pass runs, and with what LDS.  Host-only arithmetic on plain values: no device code of its own, nothing of
// the engine (tests/host/pass_plan_check.cpp runs it alone; the kernels call the layout helpers marked MHIP_PLAN_HD).
//
// The engine describes the lists it holds and the pass it is asked for in a PassShape; plan_pass() answers with a PassPlan, and the
// launch does what the plan says.  Nothing here is state: the same shape gives the same plan, and a question ("could this step be one
// launch?") is the same call as the launch's own.
//
//   form          taken when                                                         LDS
//   GROUP_SPLIT   fp32 plain pass over an inner list that has its group-split form    gs_lds_bytes(q_lds) per group, q_lds = ⌈tile / GS⌉ + 1
//   PACKED        fp32 one-type LJ, scaled entries, no special pairs, tile + 1 < 4097  x[] y[] z[] of `soa` dwords (+ 64) | j-split reduction
//   GENERIC       everything else: energy, per-atom parameters, Coulomb, segments     (tile + 1) records | reduction, + 32
//
// A pruning pass (dual list whose inner list is stale, no energy) walks the outer list and keeps its tables — renumbering table, scan
// scratch, wave boxes: prune_lds_bytes — behind the tile, at mark_off.  The tile is carved for the budget LESS those tables, so a tile
// that just fills the LDS is cut into segments a little earlier in a pruning pass.  The packed pruning kernel finds the table at the
// compile-time offset prune_mark_ct(stride): plan_pass computes mark_off by the same alignment of the same tile size, and the host
// test sweeps that the two agree for every launch shape.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/mollyhip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MHIP_PLAN_HD __host__ __device__
#else
#define MHIP_PLAN_HD
#endif

namespace mhip {

// dynamic LDS a kernel may ask for: the 160 KiB of a gfx950 CU (MI355X_MICROARCH.md) minus room for the kernels' static __shared__
// arrays (k_build: ≈ 1.6 KB) — the sum is what hipFuncSetAttribute / the launch are checked against
constexpr int MAX_LDS_BYTES = 160 * 1024 - 2048;
enum { LJ_OFF = 0, LJ_DIST = 1, LJ_GENERIC = 2, LJ_DIST_UNIFORM = 3 };   // UNIFORM: every atom has the same σ, ϵ
constexpr int ESHIFT_SCALED = 2;      // list entries = tile slot × 4 (kernels.h)

// ---- the LDS layout ----------------------------------------------------------------------------------------------------------------
// strides the packed loop is compiled for (odd numbers of dwords): tiles of up to stride − 1 atoms, 12·stride bytes of LDS.  The
// smallest that holds the tile is used: 36 KiB leaves room for four 512-lane blocks per CU, 48 KiB for three (measured: −12 % per pass).
constexpr int SOA_STRIDES[3] = {2049, 3073, 4097};
MHIP_PLAN_HD constexpr int lds_align16(int bytes) { return (bytes + 15) & ~15; }
MHIP_PLAN_HD constexpr int packed_tile_bytes(int soa) { return 3 * soa * 4 + 64; }      // x[], y[], z[] instead of the generic 16-byte records
// where the packed pruning pass keeps its renumbering table: right behind the three tile arrays
MHIP_PLAN_HD constexpr int prune_mark_ct(int soa) { return lds_align16(packed_tile_bytes(soa)); }
// dynamic LDS a PRUNE pass needs behind its tile: the renumbering table (2 bytes per tile atom of a segment), scan scratch, eight boxes,
// the atoms' row counts (lane order) and the destination waves' row counts (+ the 16 byte-permute selectors of the row compaction)
MHIP_PLAN_HD inline size_t prune_lds_bytes(int t_seg, int nthr) { return (size_t)(((t_seg + 8) & ~7) * 2) + ((size_t)nthr + 4) * 4 + 8 * 8 * 4 + ((size_t)nthr + 64) * 4 + 16 * 8 + 32; }

// one group of the group-split pass: its share of the tile as float4 + float2 records | its waves' reduction
inline size_t gs_lds_bytes(int q_lds, int BI, int JSW) { return std::max((size_t)(q_lds + 1) * (16 + 8), (size_t)JSW * 3 * BI * 4) + 64; }
// k_regroup: what the launch sets aside for staging a block's new list, behind its two count tables
inline int regroup_list_bytes(int BI, int JS, int R_cap) { return (int)std::min<size_t>((size_t)MAX_LDS_BYTES - (size_t)JS * BI * 16 - 64, (size_t)JS * R_cap * BI * 8); }

// the block pass: records of `real` bytes per coordinate (4 coordinates, + σ and ϵ with per-atom LJ) | the j-split reduction | a double per atom
inline size_t block_reduction_bytes(int BI, int JS, size_t real) { return (size_t)JS * 4 * BI * real; }
inline size_t tile_record_bytes(bool per_atom_lj, size_t real) { return 4 * real + (per_atom_lj ? 2 * real : 0); }
inline size_t force_lds_bytes(int t_lds, int BI, int JS, bool per_atom_lj, size_t real) {
    return std::max(std::max((size_t)(t_lds + 1) * tile_record_bytes(per_atom_lj, real), block_reduction_bytes(BI, JS, real)), (size_t)BI * sizeof(double)) + 32;
}
// the whole tile if it fits the budget, else segments of the budget's size (an even number of atoms, at least two).
// reserve: bytes the pass places behind the tile; it shrinks the budget only while that leaves more than 8 KiB.
struct TileCarve { bool segmented; int t_lds; size_t bytes; };
inline TileCarve carve_tile(int tile_max, size_t budget, size_t reserve, int BI, int JS, bool per_atom_lj, size_t real) {
    budget = std::min<size_t>(budget, MAX_LDS_BYTES);
    if (budget > reserve + 8192) budget -= reserve;
    const size_t per_atom = tile_record_bytes(per_atom_lj, real);
    const size_t fixed = std::max(block_reduction_bytes(BI, JS, real), (size_t)BI * sizeof(double)) + 64;
    int fit = (int)((budget > fixed + 2 * per_atom ? budget - fixed : 2 * per_atom) / per_atom) - 1;
    fit = std::max(fit & ~1, 2);
    TileCarve c;
    c.segmented = tile_max > fit;
    c.t_lds = c.segmented ? fit : std::max(tile_max, 1);
    c.bytes = force_lds_bytes(c.t_lds, BI, JS, per_atom_lj, real);
    return c;
}

// ---- the question --------------------------------------------------------------------------------------------------------------------
struct PassShape {
    // the system and its launch shape
    bool fp32 = true; int ljm = LJ_OFF, coulm = MHIP_COUL_NONE;
    bool minimg = false; int n_special = 0, eshift = 0; bool lj_c12 = false;      // lj_c12: the packed loop's constants are in the normal fp32 range
    int BI = 64, JS = 1, T_cap = 16;
    size_t lds_budget = MAX_LDS_BYTES;      // MOLLYHIP_LDS_BUDGET_KB, in bytes
    // the lists
    bool dual = false, inner_valid = false;
    int max_tile = 0, max_tile_in = 0;      // the largest tile of the outer (or only) list | of the inner list
    int gs = 0; bool gs_list_current = false;      // groups per block, 0: no group-split passes | the group-split list was dealt from the current inner list
    int64_t n_ghost = 0;
    // the request
    bool energy = false; int part = 0;      // part: 0 every block, 1 / 2 the blocks without / with ghost atoms in their tile
    bool allow_gs = false, own_frc = false;      // own_frc: the forces go to an array of the caller's
    bool step = false, halo = false, fuse_step = true;      // the fused step is asked for | of a ghosted sub-domain | MOLLYHIP_FUSE_STEP
    // Σ m v of the launch before, if its removal is still pending: 0 none, 1 subtract v_cm, 2 re-sum cm_n per-block partials
    int cm_mode = 0, cm_n = 0; bool in_step_loop = false;      // in_step_loop: inside a device step loop, whose next launch reads the sum
};

// ---- the answer ----------------------------------------------------------------------------------------------------------------------
enum class PassForm { GROUP_SPLIT, PACKED, GENERIC };
enum class PassCapacity { OK, TILE, PRUNE };      // what does not fit the LDS, if anything
struct PassPlan {
    PassForm form = PassForm::GENERIC;
    bool prune = false, use_inner = false;      // the pass prunes the outer list into the inner one | walks the inner list
    int tile_max = 0;                           // the largest tile of the list it walks
    bool segmented = false; int tile_lds = 0;   // the tile is staged in segments | of this many atoms (unsegmented: the whole tile)
    int soa = 0;                                // PACKED: the stride of x[] / y[] / z[]
    size_t lds_bytes = 0;                       // dynamic LDS of the launch, prune tables included
    int mark_off = 0;                           // prune: byte offset of the renumbering table
    int q_lds = 0;                              // GROUP_SPLIT: tile slots per group
    bool can_step = false;                      // the pass may integrate in its epilogue
    bool steps = false;                         // … and does: the fused step was asked for
    bool cm_slot = false;                       // a workgroup of this launch can sum Σ m v partials into one
    bool cm_fin = false;                        // … and sums the pending ones of the launch before
    PassCapacity capacity = PassCapacity::OK;
    int tile_segments() const { return segmented ? (std::max(tile_max, 1) + std::max(tile_lds, 1) - 1) / std::max(tile_lds, 1) : 1; }
};
inline const char* capacity_message(PassCapacity c) {
    return c == PassCapacity::TILE ? "force-kernel LDS carve-up exceeds 160 KiB" : c == PassCapacity::PRUNE ? "prune pass LDS carve-up exceeds 160 KiB" : "";
}

// the passes the packed fp32 one-type loop can run
inline bool packed_kind(const PassShape& s) {
    return s.fp32 && s.ljm == LJ_DIST_UNIFORM && s.coulm == MHIP_COUL_NONE && !s.energy && !s.minimg && s.n_special == 0 && s.eshift == ESHIFT_SCALED && s.lj_c12;
}
// the smallest stride that holds a tile of tile_max atoms + sentinel, 0: none does
inline int packed_stride(int tile_max) {
    for (int k = 0; k < 3; ++k) if (tile_max + 1 < SOA_STRIDES[k]) return SOA_STRIDES[k];
    return 0;
}

// the tile of a block pass over a list whose largest tile is tile_max, into p (also: what the engine reports for a list no pass has walked yet)
inline void plan_tile(PassPlan& p, const PassShape& s, int tile_max, size_t reserve = 0) {
    const size_t real = s.fp32 ? sizeof(float) : sizeof(double);
    const TileCarve c = carve_tile(tile_max, s.lds_budget, reserve, s.BI, s.JS, s.ljm == LJ_DIST || s.ljm == LJ_GENERIC, real);
    p.tile_max = tile_max; p.segmented = c.segmented; p.tile_lds = c.t_lds; p.lds_bytes = c.bytes;
    if (c.bytes > (size_t)MAX_LDS_BYTES) p.capacity = PassCapacity::TILE;
}

inline PassPlan plan_pass(const PassShape& s) {
    PassPlan p;
    p.use_inner = s.dual && s.inner_valid;
    p.prune = s.dual && !s.inner_valid && !s.energy;
    p.tile_max = p.use_inner ? s.max_tile_in : s.max_tile;
    const bool whole = !s.energy && s.part == 0 && !s.own_frc;      // a plain pass over every block into the engine's force array
    // inside a device step loop the Σ m v partials of the launch before become one partial here, unless this launch integrates (its head workgroup sums them then)
    auto hand_over = [&] {
        p.cm_slot = !s.energy && s.n_ghost == 0 && s.part == 0 && !p.steps;
        p.cm_fin = p.cm_slot && s.in_step_loop && s.cm_mode == 2 && s.cm_n > 1 && s.cm_n <= 65536;
    };
    // a plain pass over an inner list that has its group-split form (made right behind the prune that wrote it)
    if (s.fp32 && s.allow_gs && s.gs > 0 && p.use_inner && whole && s.gs_list_current) {
        const int q_lds = (s.max_tile_in + s.gs - 1) / s.gs + 1;      // (max_tile_in = max_tile while the outer list stands in)
        const size_t lds = gs_lds_bytes(q_lds, s.BI, s.JS / s.gs);
        if (lds <= (size_t)MAX_LDS_BYTES / s.gs) {
            p.form = PassForm::GROUP_SPLIT; p.q_lds = q_lds; p.lds_bytes = lds;
            hand_over();
            return p;
        }
    }
    plan_tile(p, s, p.tile_max, p.prune ? prune_lds_bytes(std::min(s.T_cap, s.max_tile + 1), s.BI * s.JS) + 16 : 0);
    if (p.capacity != PassCapacity::OK) return p;
    p.soa = (packed_kind(s) && !p.segmented) ? packed_stride(p.tile_max) : 0;
    if (p.soa) {
        p.form = PassForm::PACKED;
        p.lds_bytes = std::max((size_t)packed_tile_bytes(p.soa), block_reduction_bytes(s.BI, s.JS, sizeof(float)) + 32);
    }
    if (p.prune) {
        p.mark_off = lds_align16((int)p.lds_bytes);
        p.lds_bytes = (size_t)p.mark_off + prune_lds_bytes(p.tile_lds, s.BI * s.JS);
        if (p.lds_bytes > (size_t)MAX_LDS_BYTES) { p.capacity = PassCapacity::PRUNE; return p; }
    }
    p.can_step = s.fuse_step && p.soa != 0 && p.use_inner && !p.prune && whole && (s.n_ghost == 0 || s.halo) && s.cm_mode != 1;
    p.steps = s.step && p.can_step;
    hand_over();
    return p;
}

}  // namespace mhip
