// Stand-alone check of molly.jl_amd/csrc/pass_plan.h (tests/test_pass_plan_host.py compiles and runs it): known answers of the plan —
// stride bands, what loses the packed loop, where a tile is cut into segments, the prune reserve, the group-split bound, who may
// integrate — then a deterministic sweep of the layout properties every launch relies on.  Exit status 0 = pass.
#include <cstdint>
#include <cstdio>

#include "pass_plan.h"

using namespace mhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const char* form_name(PassForm f) { return f == PassForm::GROUP_SPLIT ? "GROUP_SPLIT" : f == PassForm::PACKED ? "PACKED" : "GENERIC"; }

// an fp32 one-type LJ fluid in 256 x 2 blocks with a valid inner list of `tile` atoms at most: the plain pass is the packed loop
static PassShape one_type(int tile) {
    PassShape s;
    s.fp32 = true; s.ljm = LJ_DIST_UNIFORM; s.coulm = MHIP_COUL_NONE; s.eshift = ESHIFT_SCALED; s.lj_c12 = true;
    s.BI = 256; s.JS = 2; s.T_cap = 16380;
    s.dual = true; s.inner_valid = true; s.max_tile = tile; s.max_tile_in = tile;
    return s;
}
// the carve-up alone: a single list (no prune, no inner list), entries unscaled so that no shape is the packed kind
static PassShape single_list(bool fp32, int ljm, int tile, size_t budget) {
    PassShape s;
    s.fp32 = fp32; s.ljm = ljm; s.BI = 256; s.JS = 2; s.T_cap = 16380; s.lds_budget = budget; s.max_tile = tile;
    return s;
}

static void known_answers() {
    {   // the packed stride bands: tile + sentinel must be BELOW the stride
        const int tile[6] = {2047, 2048, 3071, 3072, 4095, 4096}, soa[6] = {2049, 3073, 3073, 4097, 4097, 0};
        for (int k = 0; k < 6; ++k) {
            const PassPlan p = plan_pass(one_type(tile[k]));
            CHECK(p.soa == soa[k] && p.form == (soa[k] ? PassForm::PACKED : PassForm::GENERIC) && !p.segmented && p.tile_lds == tile[k], "tile %d: soa %d form %s", tile[k], p.soa, form_name(p.form));
            CHECK(p.lds_bytes == (soa[k] ? (size_t)12 * soa[k] + 64 : (size_t)(tile[k] + 1) * 16 + 32), "tile %d: lds %zu", tile[k], p.lds_bytes);
            CHECK(p.can_step == (soa[k] != 0) && p.use_inner && !p.prune, "tile %d: can_step %d", tile[k], (int)p.can_step);
        }
    }
    {   // each of these alone loses the packed loop, and with it the fused step
        PassShape v[7]; for (PassShape& s : v) s = one_type(1500);
        v[0].energy = true; v[1].minimg = true; v[2].n_special = 1; v[3].eshift = 0; v[4].lj_c12 = false; v[5].fp32 = false; v[6].coulm = MHIP_COUL_REACTION_FIELD;
        const PassPlan base = plan_pass(one_type(1500));
        CHECK(base.form == PassForm::PACKED && base.can_step && base.soa == 2049, "base: %s", form_name(base.form));
        for (int k = 0; k < 7; ++k) { const PassPlan p = plan_pass(v[k]); CHECK(p.form == PassForm::GENERIC && p.soa == 0 && !p.can_step, "variant %d: %s can_step %d", k, form_name(p.form), (int)p.can_step); }
    }
    {   // the segmentation edge, from the carve-up rule by hand: fit = ((budget − fixed) / record − 1) & ~1, fixed = max(JS·4·BI·real, 8·BI) + 64 = 8 256 (fp32) | 16 448 (fp64)
        struct Row { bool fp32; int ljm; size_t budget; int fit; } rows[8] = {
            {true, LJ_DIST, (size_t)MAX_LDS_BYTES, 6396}, {true, LJ_DIST_UNIFORM, (size_t)MAX_LDS_BYTES, 9594}, {false, LJ_DIST, (size_t)MAX_LDS_BYTES, 3026}, {false, LJ_DIST_UNIFORM, (size_t)MAX_LDS_BYTES, 4540},
            {true, LJ_DIST, 17 * 1024, 380}, {true, LJ_DIST_UNIFORM, 17 * 1024, 570}, {false, LJ_DIST, 17 * 1024, 18}, {false, LJ_DIST_UNIFORM, 17 * 1024, 28}};
        for (const Row& r : rows) {
            const size_t rec = (r.fp32 ? 4 : 8) * (r.ljm == LJ_DIST ? 6 : 4), red = (size_t)2 * 4 * 256 * (r.fp32 ? 4 : 8);
            const PassPlan a = plan_pass(single_list(r.fp32, r.ljm, r.fit, r.budget)), b = plan_pass(single_list(r.fp32, r.ljm, r.fit + 1, r.budget));
            CHECK(!a.segmented && a.tile_lds == r.fit && a.tile_segments() == 1 && a.lds_bytes == std::max((size_t)(r.fit + 1) * rec, red) + 32 && a.lds_bytes <= r.budget, "fp32 %d ljm %d budget %zu: tile_lds %d lds %zu", (int)r.fp32, r.ljm, r.budget, a.tile_lds, a.lds_bytes);
            CHECK(b.segmented && b.tile_lds == r.fit && b.tile_segments() == 2 && b.lds_bytes == a.lds_bytes && b.form == PassForm::GENERIC, "fp32 %d ljm %d budget %zu: tile + 1: segmented %d tile_lds %d", (int)r.fp32, r.ljm, r.budget, (int)b.segmented, b.tile_lds);
        }
        // the budget is the engine's to set, at most the device's
        CHECK(plan_pass(single_list(true, LJ_DIST, 6397, (size_t)1 << 30)).tile_lds == 6396, "budget above the device's");
    }
    {   // the prune reserve (tables of a 1 001-atom segment and 512 lanes, + 16: 6 816 bytes) shrinks the budget only while budget > reserve + 8 192
        PassShape s = single_list(true, LJ_DIST, 1000, 17 * 1024); s.dual = true;
        CHECK(prune_lds_bytes(1001, 512) + 16 == 6816, "reserve %zu", prune_lds_bytes(1001, 512) + 16);
        const PassPlan a = plan_pass(s);       // 17 408 − 6 816 = 10 592 → (10 592 − 8 256) / 24 − 1 → 96
        s.lds_budget = 14 * 1024;
        const PassPlan b = plan_pass(s);       // 14 336 <= 15 008: not shrunk → (14 336 − 8 256) / 24 − 1 → 252
        CHECK(a.prune && a.segmented && a.tile_lds == 96 && b.prune && b.segmented && b.tile_lds == 252, "tile_lds %d, %d", a.tile_lds, b.tile_lds);
        CHECK(a.mark_off == lds_align16((int)(8192 + 32)) && a.lds_bytes == (size_t)a.mark_off + prune_lds_bytes(96, 512), "mark_off %d lds %zu", a.mark_off, a.lds_bytes);
        s.energy = true;
        CHECK(!plan_pass(s).prune && !plan_pass(s).use_inner, "an energy pass never prunes");
    }
    {   // the group-split pass: every condition, and its LDS bound — 64 x 16 in four groups: (q + 1)·24 + 64 <= 40 448 ⇔ q <= 1 681 ⇔ tile <= 6 720
        PassShape g;
        g.fp32 = true; g.ljm = LJ_DIST; g.coulm = MHIP_COUL_REACTION_FIELD; g.BI = 64; g.JS = 16; g.T_cap = 16380;
        g.dual = true; g.inner_valid = true; g.max_tile = 8000; g.max_tile_in = 6720; g.gs = 4; g.gs_list_current = true; g.allow_gs = true;
        const PassPlan p = plan_pass(g);
        CHECK(p.form == PassForm::GROUP_SPLIT && p.q_lds == 1681 && p.lds_bytes == 40432 && p.lds_bytes == gs_lds_bytes(1681, 64, 4) && p.tile_max == 6720 && !p.can_step, "%s q_lds %d lds %zu", form_name(p.form), p.q_lds, p.lds_bytes);
        PassShape v[8]; for (PassShape& s : v) s = g;
        v[0].max_tile_in = 6721; v[1].allow_gs = false; v[2].inner_valid = false; v[3].part = 2; v[4].own_frc = true; v[5].gs_list_current = false; v[6].energy = true; v[7].gs = 0;
        CHECK(gs_lds_bytes(1682, 64, 4) > (size_t)MAX_LDS_BYTES / 4, "bound");
        for (int k = 0; k < 8; ++k) CHECK(plan_pass(v[k]).form == PassForm::GENERIC, "variant %d: %s", k, form_name(plan_pass(v[k]).form));
    }
    {   // who may integrate: the packed pass over the inner list, every block, the engine's force array, ghosts only in the halo form, Σ m v not to be subtracted
        PassShape v[8]; for (PassShape& s : v) s = one_type(1500);
        v[0].inner_valid = false; v[1].part = 1; v[2].own_frc = true; v[3].n_ghost = 10; v[4].cm_mode = 1; v[5].fuse_step = false; v[6].dual = false; v[7].max_tile_in = 4096;
        for (int k = 0; k < 8; ++k) { PassShape s = v[k]; s.step = true; const PassPlan p = plan_pass(s); CHECK(!p.can_step && !p.steps, "variant %d", k); }
        CHECK(plan_pass(v[0]).prune && plan_pass(v[0]).form == PassForm::PACKED, "the pruning pass of a one-type fluid is packed, and does not integrate");
        PassShape h = one_type(1500); h.n_ghost = 10; h.halo = true; h.step = true; h.cm_mode = 2; h.cm_n = 100;
        CHECK(plan_pass(h).can_step && plan_pass(h).steps, "halo");
        h.step = false;
        CHECK(plan_pass(h).can_step && !plan_pass(h).steps, "asked without the request");
    }
    {   // the Σ m v hand-over: inside a step loop, partials pending, a plain pass over every block without ghosts that does not integrate itself
        PassShape s = one_type(1500); s.in_step_loop = true; s.cm_mode = 2; s.cm_n = 250;
        CHECK(plan_pass(s).cm_fin && plan_pass(s).cm_slot, "plain pass");
        PassShape v[8]; for (PassShape& q : v) q = s;
        v[0].step = true; v[1].energy = true; v[2].part = 1; v[3].n_ghost = 5; v[4].cm_n = 1; v[5].cm_n = 65537; v[6].cm_mode = 0; v[7].in_step_loop = false;
        for (int k = 0; k < 8; ++k) CHECK(!plan_pass(v[k]).cm_fin, "variant %d", k);
        CHECK(!plan_pass(v[0]).cm_slot && plan_pass(v[7]).cm_slot, "cm_slot");
    }
}

// ---- sweep -----------------------------------------------------------------------------------------------------------------------
static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg_state >> 33); }
static bool coin() { return (rnd() & 1u) != 0u; }
static bool rarely() { return (rnd() & 7u) == 0u; }

static PassShape random_shape() {
    PassShape s;
    s.fp32 = coin();
    static const int LJM[4] = {LJ_OFF, LJ_DIST, LJ_GENERIC, LJ_DIST_UNIFORM};
    s.ljm = coin() ? LJ_DIST_UNIFORM : LJM[rnd() % 4];
    s.coulm = coin() ? MHIP_COUL_NONE : (int)(rnd() % 4);
    s.minimg = rarely(); s.n_special = rarely() ? 1 : 0; s.eshift = rarely() ? 0 : ESHIFT_SCALED; s.lj_c12 = !rarely();
    const int lanes = s.fp32 ? 1024 : 512;
    s.BI = 64 << (rnd() % 3);
    int njs = 0; for (int js = 1; s.BI * js <= lanes; js *= 2) ++njs;
    s.JS = 1 << (rnd() % njs);
    s.max_tile = 1 + (int)(rnd() % 16380);
    s.max_tile_in = coin() ? s.max_tile : 1 + (int)(rnd() % s.max_tile);
    s.T_cap = std::min(16380, ((s.max_tile + (int)(rnd() % 64)) + 3) & ~3);
    s.lds_budget = (size_t)(17 + rnd() % 144) * 1024;
    s.dual = !rarely(); s.inner_valid = coin();
    s.n_ghost = rarely() ? 100 : 0;
    s.gs = (s.fp32 && s.n_ghost == 0 && s.JS % 4 == 0 && s.BI * (s.JS / 4) == 256 && coin()) ? 4 : 0; s.gs_list_current = coin();      // (k_forces_gs: 256 lanes, single domain)
    s.energy = rarely(); s.part = rarely() ? 1 + (int)(rnd() % 2) : 0; s.allow_gs = coin(); s.own_frc = rarely();
    s.step = coin(); s.halo = s.n_ghost > 0 && coin(); s.fuse_step = !rarely();
    s.cm_mode = (int)(rnd() % 3); s.cm_n = (int)(rnd() % 4) == 0 ? 1 : 1 + (int)(rnd() % 70000); s.in_step_loop = coin();
    return s;
}

static bool same(const PassPlan& a, const PassPlan& b) {
    return a.form == b.form && a.prune == b.prune && a.use_inner == b.use_inner && a.tile_max == b.tile_max && a.segmented == b.segmented && a.tile_lds == b.tile_lds && a.soa == b.soa &&
           a.lds_bytes == b.lds_bytes && a.mark_off == b.mark_off && a.q_lds == b.q_lds && a.can_step == b.can_step && a.steps == b.steps && a.cm_slot == b.cm_slot && a.cm_fin == b.cm_fin && a.capacity == b.capacity;
}

static void sweep(int n) {
    int forms[3] = {0, 0, 0}, n_prune = 0, n_seg = 0, n_step = 0, n_cap = 0;
    for (int it = 0; it < n; ++it) {
        const PassShape s = random_shape();
        const PassPlan p = plan_pass(s);
        CHECK(same(p, plan_pass(s)), "input %d: not pure", it);
        if (p.capacity != PassCapacity::OK) { ++n_cap; continue; }
        ++forms[(int)p.form]; n_prune += p.prune; n_seg += p.segmented; n_step += p.can_step;
        CHECK(p.lds_bytes <= (size_t)MAX_LDS_BYTES, "input %d: lds %zu", it, p.lds_bytes);
        if (p.form == PassForm::GROUP_SPLIT) { CHECK(p.lds_bytes * s.gs <= (size_t)MAX_LDS_BYTES && p.q_lds * s.gs > p.tile_max && !p.prune && p.use_inner && !p.can_step, "input %d: group-split", it); continue; }
        const size_t real = s.fp32 ? 4 : 8, rec = (s.ljm == LJ_DIST || s.ljm == LJ_GENERIC) ? 6 * real : 4 * real, red = (size_t)s.JS * 4 * s.BI * real;
        if (p.segmented) CHECK(p.soa == 0 && p.tile_lds >= 2 && p.tile_lds % 2 == 0 && p.tile_lds < p.tile_max, "input %d: segments of %d", it, p.tile_lds);
        else CHECK(p.tile_lds == p.tile_max, "input %d: tile_lds %d of %d", it, p.tile_lds, p.tile_max);
        const size_t tile_end = p.soa ? (size_t)12 * p.soa : (size_t)(p.tile_lds + 1) * rec;
        const size_t front = p.prune ? (size_t)p.mark_off : p.lds_bytes;      // tile | reduction, in front of the prune tables
        CHECK(front >= tile_end && front >= red && front >= (size_t)8 * s.BI, "input %d: front %zu tile %zu reduction %zu", it, front, tile_end, red);
        if (p.soa) CHECK(p.form == PassForm::PACKED && p.tile_max + 1 < p.soa && (p.soa == 2049 || p.soa == 3073 || p.soa == 4097), "input %d: soa %d tile %d", it, p.soa, p.tile_max);
        else CHECK(p.form == PassForm::GENERIC, "input %d", it);
        if (p.prune) {
            CHECK(p.mark_off % 16 == 0 && !p.use_inner && p.lds_bytes == (size_t)p.mark_off + prune_lds_bytes(p.tile_lds, s.BI * s.JS), "input %d: mark_off %d", it, p.mark_off);
            if (p.soa) CHECK(p.mark_off == prune_mark_ct(p.soa), "input %d: the packed pruning kernel looks for its table at %d, the plan puts it at %d", it, prune_mark_ct(p.soa), p.mark_off);
        } else CHECK(p.mark_off == 0, "input %d", it);
        if (p.can_step) CHECK(p.form == PassForm::PACKED && !p.segmented && !p.prune && p.use_inner, "input %d: can_step", it);
        CHECK((!p.steps || p.can_step) && (!p.cm_fin || (p.cm_slot && !p.steps)), "input %d: steps / cm_fin", it);
    }
    std::printf("sweep: %d inputs: group-split %d, packed %d, generic %d, over capacity %d | pruning %d, segmented %d, may integrate %d\n", n, forms[0], forms[1], forms[2], n_cap, n_prune, n_seg, n_step);
    CHECK(forms[0] > 100 && forms[1] > 1000 && forms[2] > 1000 && n_prune > 1000 && n_seg > 1000 && n_step > 100, "the sweep missed a form");
}

int main() {
    known_answers();
    sweep(200000);
    std::printf(failures ? "%d FAILURES\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
