// step_plan.h — which launch closes an MD step, and what the force pass is asked to do on the way.  Host-only arithmetic on plain values:
// no HIP header, nothing of the engine (tests/host/step_plan_check.cpp runs it alone), no state, no allocation, everything by value.
//
// Per run the engine describes its loop in a RunShape; plan_run() answers with a RunPlan (one member of the engine while the loop runs:
// async_ok() and pass_shape() read it).  Per step the loop fills a StepShape twice — the lists change across the force pass, and whether a
// launch measures the next list check is decided on both sides of it on purpose:
//
//   resolve_due()    is the check a launch measured read at the top of this step?
//   plan_request()   before the pass: cm, th, and what goes into the pass's request (step, gcv, measure)
//   plan_stage()     behind the pass, if it did not integrate: the launch form, its blocks, where Σ m v goes, the bookkeeping
//   plan_open()      the launch that opens a run (or, in the two-launch form, every step)
//
//   form          launches                                              taken when
//   VV1           k_vv1                                                 opening: first kick + drift (plain block rule)
//   VV2           k_vv2<cm>                                             two-launch form (Andersen, the stage entry points): the closing kick; Σ m v → first half | caller
//   VV_MID        k_vv_mid<cm, last>                                    fused VV and the stepwise ghosted step: closing kick (+ next kick and drift unless last)
//   CON_STEP      k_con_step mode 0 | 1 | 2 | 3                         constraints or hosted sites: opening | mid-run | last step | the Langevin update
//   THERMO        k_vv_close + k_vv_open    (k_con_step 2, then 0)      a step on which a rescaling thermostat applies
//   THERMO_LAST   k_vv_close + k_scale_vel  (k_con_step 2, then scale)  … that is the run's last
//   LANGEVIN      launch_langevin                                       the Langevin update without constraints (never measures)
//   NONE          —                                                     the force pass integrated (k_forces STEP, k_gather_collect_vv)
//
// Blocks: a stage launch writes one Σ m v partial {Px, Py, Pz, M} per block into a half of the engine's buffer, CM_HALF_PARTS entries — both
// block rules and the work-item rule are bounded by it.  With the caller's partial buffer every one of its slots gets a block.
#pragma once
#include <algorithm>
#include <cstdint>

namespace mhip {

constexpr int CM_HALF_PARTS = 1024;      // Σ m v partials of one half of cm_step
// one 256-lane block per 256 atoms, as many as a half holds
inline int stage_blocks(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, CM_HALF_PARTS); }
// every block re-sums the previous step's per-block Σ m v partials (32 bytes each), so fewer, longer blocks pay: 1024 blocks re-read 32 MB from L2 per launch —
// more than the 21 MB of atoms of the 256k-atom fluid (13.0 → 10.0 µs with 256 blocks; 1M atoms: 21.2 → 20.2 µs with 512, 21.8 with 256)
inline int stage_blocks_long(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, std::max<int64_t>(256, std::min<int64_t>(512, n / 2048))); }
// k_con_step: one lane per work item
inline int item_blocks(int64_t n_items, int per_block) { return (int)std::max<int64_t>(1, std::min<int64_t>((n_items + per_block - 1) / per_block, CM_HALF_PARTS)); }

// ---- per run -------------------------------------------------------------------------------------------------------------------------
enum class Loop { VV, LANGEVIN, STEPWISE };      // mhip_vv_run / one brick of mhip_domain_run | mhip_langevin_run | one ghosted step per call (mhip_vv_halo_mid)
struct RunShape {
    Loop loop = Loop::VV;
    bool andersen = false, items = false;      // Andersen coupling | constraints or hosted sites (k_con_step steps them)
    bool bonded = false, pme = false, dual = false;
    bool fuse_step = true, fuse_gcv = true;    // MOLLYHIP_FUSE_STEP, MOLLYHIP_FUSE_GATHER_VV as read when the context was made
};
enum class PassKick { NONE, STEP, GCV };       // which force launch may integrate: none | the packed pair pass | the gather-collect launch of a small system
struct RunPlan {                               // (the default: no loop — the two-launch step of the stage entry points)
    Loop loop = Loop::VV;
    bool items = false;
    bool fused = false;                        // one integrator launch between consecutive force passes (else k_vv1 … k_vv2 per step)
    bool pre = false;                          // the list upkeep of a cadence step runs in front of its force pass, which prunes on the way
    PassKick kick = PassKick::NONE;
    bool async = false;                        // list checks are measured inside the launches that make the coordinates
    bool pass_sums_cm = false;                 // the pair pass in between sums the pending Σ m v partials into one
};
inline RunPlan plan_run(const RunShape& s) {
    RunPlan p;
    p.loop = s.loop; p.items = s.items;
    // (k_con_step updates whole clusters: no force launch integrates then; a force chain with only one of bonded terms and PME has no launch that can)
    const PassKick kick = s.items ? PassKick::NONE : (s.bonded && s.pme) ? PassKick::GCV : (!s.bonded && !s.pme) ? PassKick::STEP : PassKick::NONE;
    switch (s.loop) {
    case Loop::VV:          // the Andersen thermostat needs v_n between the kicks: the two-launch form then
        p.fused = !s.andersen; p.pre = s.dual; p.kick = p.fused ? kick : PassKick::NONE; p.async = p.fused; p.pass_sums_cm = p.fused;
        break;
    case Loop::LANGEVIN:    // a step is complete in itself: every step's pass may integrate; no check is measured in front of an Andersen redraw
        p.fused = true; p.kick = kick; p.pass_sums_cm = kick == PassKick::GCV && s.fuse_gcv;
        p.async = (p.pass_sums_cm || s.items || (kick == PassKick::STEP && s.fuse_step)) && !s.andersen;
        break;
    case Loop::STEPWISE:
        p.fused = true; p.pre = s.dual;
        break;
    }
    return p;
}

// ---- per step ------------------------------------------------------------------------------------------------------------------------
struct StepShape {
    int64_t step = 0; bool last = false;
    int remove_cm_every = 0, thermo_every = 0;      // 0: never | the thermostat's n_steps, 0: none
    bool due = false, due_next = false;             // ListPolicy::check_due of step | of step + 1
    bool async_ok = false, trk_issued = false;
    int64_t n_atoms = 0; int item_blocks = 1;       // owned atoms | the blocks of a k_con_step launch
    int n_parts_last = 0;                           // the caller's Σ m v partial buffer for the last step: its slots, 0: none
    bool solo = true;                               // STEPWISE: no peers, the partials of the launch before are the whole sum
};
// a check measured by the launch of step trk_step is read one step later — two in the Langevin loop, which is one force pass behind (its update of step s makes x_s)
inline bool resolve_due(const RunPlan& r, int64_t step, int64_t trk_step) { return r.loop == Loop::LANGEVIN ? (!r.async || step > trk_step + 1) : step > trk_step; }

struct StepRequest {
    bool cm = false, th = false;                    // this step removes the centre-of-mass motion | a rescaling thermostat applies behind it
    bool step = false, gcv = false, measure = false;      // PassReq: the packed pass integrates | the gather-collect launch does | … and measures the next check
};
inline bool step_cm(const StepShape& s) { return s.remove_cm_every != 0 && s.step % s.remove_cm_every == 0; }
inline bool step_th(const RunPlan& r, const StepShape& s) { return r.loop == Loop::VV && s.thermo_every > 0 && s.step % s.thermo_every == 0; }
inline StepRequest plan_request(const RunPlan& r, const StepShape& s) {
    StepRequest q;
    q.cm = step_cm(s); q.th = step_th(r, s);
    const bool can_measure = r.async && s.async_ok && !s.trk_issued;
    if (r.loop == Loop::LANGEVIN) {       // the update of step s makes x_s: the check of s itself, every step of the run alike
        q.measure = can_measure && s.due;
        q.step = r.kick == PassKick::STEP; q.gcv = r.kick == PassKick::GCV;
    } else if (r.loop == Loop::VV && r.fused) {
        // the launch of step s makes x_(s+1): the check of s + 1.  λ needs Σ m v² of ALL atoms between the kicks, and the last step keeps its closing kick: no force launch integrates there
        q.measure = !s.last && can_measure && s.due_next;
        const bool integrate = !s.last && !q.th;
        q.step = integrate && r.kick == PassKick::STEP;
        q.gcv = integrate && r.kick == PassKick::GCV && (r.pre || !s.due);      // (a re-sort behind the pass would want the total force array)
    }
    return q;
}

// the fused step of a ghosted sub-domain (mhip_domain_run with peers): the packed pass must integrate; whether it measures is the collective check's decision
inline StepRequest fused_halo_request(bool cm, bool measure) { StepRequest q; q.cm = cm; q.step = true; q.measure = measure; return q; }

enum class StageForm { NONE, VV1, VV2, VV_MID, CON_STEP, THERMO, THERMO_LAST, LANGEVIN };
enum class CmDest { NONE, ENGINE_HALF, ENGINE_FIRST, CALLER };      // a half of cm_step in turn | its first half (the reader is a later call) | the caller's partial buffer
struct StagePlan {
    StageForm form = StageForm::NONE;
    int con_mode = -1;                    // CON_STEP: the mode; THERMO*: 2 when k_con_step closes (and opens, mode 0), −1: k_vv_close / k_vv_open
    bool cm = false, last = false;
    bool measure = false; int64_t check_step = 0;      // the launch takes the maxima of a list check | of this step's coordinates
    int nb = 0;
    CmDest dest = CmDest::NONE;
    bool flip = false;                    // ENGINE_HALF: the next launch writes the other half
    bool repend = false;                  // the partials are registered as the pending Σ m v removal (not on thermostat steps: removed with the scale; not the caller's)
    bool refresh_behind = false;          // no dual list to prune on the way: the cadence refresh of this step comes behind the pass (VV: in front of the stage, after folding the side forces)
};
// q: the request this step's pass was planned with.  s: re-read behind the pass in the VV loop (a prune inside the pass makes the lists checkable again);
// the Langevin loop keeps its request's measure decision, the stepwise step its cadence decision (neither is re-read)
inline StagePlan plan_stage(const RunPlan& r, const StepShape& s, const StepRequest& q, bool integrated) {
    StagePlan p;
    p.refresh_behind = !r.pre && s.due;
    if (integrated) return p;
    p.cm = q.cm; p.last = s.last;
    const bool can_measure = r.async && s.async_ok && !s.trk_issued;
    bool parts_out = false;
    switch (r.loop) {
    case Loop::VV:
        if (!r.fused) {      // every step ends: k_vv2 with the plain rule, read by the k_vv1 of a later call
            parts_out = q.cm && s.n_parts_last > 0;
            p.form = StageForm::VV2; p.last = true;
            p.nb = parts_out ? s.n_parts_last : stage_blocks(s.n_atoms);
            p.dest = !q.cm ? CmDest::NONE : parts_out ? CmDest::CALLER : CmDest::ENGINE_FIRST;
            p.repend = q.cm && !parts_out;
            return p;
        }
        parts_out = s.last && q.cm && s.n_parts_last > 0;
        p.nb = r.items ? s.item_blocks : parts_out ? s.n_parts_last : stage_blocks_long(s.n_atoms);
        p.measure = !s.last && can_measure && s.due_next; p.check_step = s.step + 1;
        p.dest = !q.cm ? CmDest::NONE : parts_out ? CmDest::CALLER : CmDest::ENGINE_HALF;
        if (q.th) { p.form = s.last ? StageForm::THERMO_LAST : StageForm::THERMO; p.con_mode = r.items ? 2 : -1; }
        else if (r.items) { p.form = StageForm::CON_STEP; p.con_mode = s.last ? 2 : 1; }
        else p.form = StageForm::VV_MID;
        p.repend = p.flip = q.cm && !parts_out && !q.th;
        break;
    case Loop::LANGEVIN:
        p.last = false;
        p.nb = r.items ? s.item_blocks : stage_blocks(s.n_atoms);
        p.dest = q.cm ? CmDest::ENGINE_HALF : CmDest::NONE;
        if (r.items) { p.form = StageForm::CON_STEP; p.con_mode = 3; p.measure = q.measure; p.check_step = s.step; }
        else p.form = StageForm::LANGEVIN;
        p.repend = p.flip = q.cm;
        break;
    case Loop::STEPWISE:     // the sum travels with the ghost message (or, solo, stays in the half the next call reads): nothing is registered
        parts_out = q.cm && s.last;
        p.form = StageForm::VV_MID;
        p.nb = parts_out ? s.n_parts_last : s.solo ? stage_blocks_long(s.n_atoms) : stage_blocks(s.n_atoms);
        p.dest = !q.cm ? CmDest::NONE : parts_out ? CmDest::CALLER : s.solo ? CmDest::ENGINE_HALF : CmDest::ENGINE_FIRST;
        p.flip = !s.last && s.solo;
        break;
    }
    return p;
}
// first kick + drift (with constraints: + RATTLE, SHAKE) on forces that are in place: once per run of n_steps in the fused form, per step in the two-launch form
inline StagePlan plan_open(const RunPlan& r, const StepShape& s, int64_t n_steps = 1) {
    StagePlan p;
    if (r.loop != Loop::VV || n_steps <= 0) return p;
    if (r.items) { p.form = StageForm::CON_STEP; p.con_mode = 0; p.nb = s.item_blocks; }
    else { p.form = StageForm::VV1; p.nb = stage_blocks(s.n_atoms); }
    return p;
}

}  // namespace mhip
