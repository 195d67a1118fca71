// Stand-alone check of molly.jl_amd/csrc/step_plan.h (tests/test_step_plan_host.py compiles and runs it): known answers — the run plans, the requests and the
// stage plans of every launch form, written down by hand from the schedule of the step loops, at the edges where it turns (first and last step, thermostat
// steps, cadence steps with and without the dual list, a check already issued, caller parts, the clamps of the block rules) — then a sweep over every
// combination of the boolean fields × loops × step positions × atom counts for the properties the engine relies on.  Exit status 0 = pass.
#include <cstdio>

#include "step_plan.h"

using namespace mhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; if (failures < 50) { std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int n_known = 0;
static RunPlan run_of(Loop loop, bool andersen, bool items, bool bonded, bool pme, bool dual, bool fuse_step = true, bool fuse_gcv = true) {
    RunShape s;
    s.loop = loop; s.andersen = andersen; s.items = items; s.bonded = bonded; s.pme = pme; s.dual = dual; s.fuse_step = fuse_step; s.fuse_gcv = fuse_gcv;
    return plan_run(s);
}
static void known_run(const char* what, const RunPlan& p, bool fused, bool pre, PassKick kick, bool async, bool sums) {
    ++n_known;
    CHECK(p.fused == fused && p.pre == pre && p.kick == kick && p.async == async && p.pass_sums_cm == sums, "%s: fused %d pre %d kick %d async %d sums %d", what, (int)p.fused, (int)p.pre, (int)p.kick,
          (int)p.async, (int)p.pass_sums_cm);
}
// the steps of the known answers: a run of steps 101 .. 160, lists checked every 10 steps
static const int EVERY = 10;
static const int64_t LAST = 160;
static StepShape at(int64_t step, int cm_every, int th_every, bool async_ok, bool trk_issued, int64_t n_atoms = 27000, int n_parts_last = 0) {
    StepShape s;
    s.step = step; s.last = step == LAST; s.remove_cm_every = cm_every; s.thermo_every = th_every;
    s.due = step % EVERY == 0; s.due_next = (step + 1) % EVERY == 0;
    s.async_ok = async_ok; s.trk_issued = trk_issued; s.n_atoms = n_atoms; s.item_blocks = 33; s.n_parts_last = n_parts_last;
    return s;
}
static void known_request(const char* what, const RunPlan& r, const StepShape& s, bool cm, bool th, bool step, bool gcv, bool measure) {
    const StepRequest q = plan_request(r, s);
    ++n_known;
    CHECK(q.cm == cm && q.th == th && q.step == step && q.gcv == gcv && q.measure == measure, "%s: cm %d th %d step %d gcv %d measure %d", what, (int)q.cm, (int)q.th, (int)q.step, (int)q.gcv, (int)q.measure);
}
struct Want { StageForm form; int con_mode; bool cm, last, measure; int64_t check_step; int nb; CmDest dest; bool flip, repend, refresh_behind; };
static void known_plan(const char* what, const StagePlan& p, const Want& w) {
    ++n_known;
    CHECK(p.form == w.form && p.con_mode == w.con_mode && p.cm == w.cm && p.last == w.last && p.measure == w.measure && (!w.measure || p.check_step == w.check_step) && p.nb == w.nb && p.dest == w.dest &&
              p.flip == w.flip && p.repend == w.repend && p.refresh_behind == w.refresh_behind,
          "%s: form %d mode %d cm %d last %d measure %d at %lld nb %d dest %d flip %d repend %d refresh %d", what, (int)p.form, p.con_mode, (int)p.cm, (int)p.last, (int)p.measure, (long long)p.check_step, p.nb,
          (int)p.dest, (int)p.flip, (int)p.repend, (int)p.refresh_behind);
}
static void known_stage(const char* what, const RunPlan& r, const StepShape& s, const Want& w) { known_plan(what, plan_stage(r, s, plan_request(r, s), false), w); }

static void known_answers() {
    const bool Y = true, N = false;
    // ---- the block rules, both sides of each clamp -------------------------------------------------------------------------------------------
    struct B { int64_t n; int plain, lng; };
    const B blocks[] = {{1, 1, 1},           {255, 1, 1},         {256, 1, 1},           {257, 2, 2},           {65536, 256, 256},     {65537, 257, 256},    {261888, 1023, 256},
                        {262144, 1024, 256}, {262145, 1024, 256}, {524288 + 1, 1024, 256}, {526336, 1024, 257}, {1048575, 1024, 511},  {1048576, 1024, 512}, {1048576 + 2048, 1024, 512},
                        {(int64_t)1 << 30, 1024, 512}};
    for (const B& b : blocks) { ++n_known; CHECK(stage_blocks(b.n) == b.plain && stage_blocks_long(b.n) == b.lng, "%lld atoms: %d and %d blocks", (long long)b.n, stage_blocks(b.n), stage_blocks_long(b.n)); }
    CHECK(CM_HALF_PARTS == 1024, "a half of the partial buffer");
    CHECK(item_blocks(0, 64) == 1 && item_blocks(64, 64) == 1 && item_blocks(65, 64) == 2 && item_blocks(64 * 1024 + 1, 64) == 1024, "work items per launch");

    // ---- per run -----------------------------------------------------------------------------------------------------------------------------
    //                                                  andersen items bonded pme dual            fused pre kick          async sums
    const RunPlan fluid = run_of(Loop::VV, N, N, N, N, Y);
    const RunPlan fluid_single = run_of(Loop::VV, N, N, N, N, N);
    const RunPlan andersen = run_of(Loop::VV, Y, N, N, N, Y);
    const RunPlan water = run_of(Loop::VV, N, Y, N, N, Y);
    const RunPlan protein = run_of(Loop::VV, N, N, Y, Y, Y);
    const RunPlan protein_single = run_of(Loop::VV, N, N, Y, Y, N);
    known_run("VV fluid", fluid, Y, Y, PassKick::STEP, Y, Y);
    known_run("VV fluid, single list", fluid_single, Y, N, PassKick::STEP, Y, Y);
    known_run("VV fluid, fuse switches off (read by the pass itself)", run_of(Loop::VV, N, N, N, N, Y, N, N), Y, Y, PassKick::STEP, Y, Y);
    known_run("VV Andersen", andersen, N, Y, PassKick::NONE, N, N);
    known_run("VV constraints", water, Y, Y, PassKick::NONE, Y, Y);
    known_run("VV bonded + PME", protein, Y, Y, PassKick::GCV, Y, Y);
    known_run("VV bonded only", run_of(Loop::VV, N, N, Y, N, Y), Y, Y, PassKick::NONE, Y, Y);
    known_run("VV PME only", run_of(Loop::VV, N, N, N, Y, N), Y, N, PassKick::NONE, Y, Y);
    const RunPlan lang_fluid = run_of(Loop::LANGEVIN, N, N, N, N, Y);
    const RunPlan lang_water = run_of(Loop::LANGEVIN, N, Y, N, N, Y);
    const RunPlan lang_protein = run_of(Loop::LANGEVIN, N, N, Y, Y, Y);
    known_run("Langevin fluid", lang_fluid, Y, N, PassKick::STEP, Y, N);
    known_run("Langevin fluid, FUSE_STEP 0", run_of(Loop::LANGEVIN, N, N, N, N, Y, N, Y), Y, N, PassKick::STEP, N, N);
    known_run("Langevin fluid, Andersen", run_of(Loop::LANGEVIN, Y, N, N, N, Y), Y, N, PassKick::STEP, N, N);
    known_run("Langevin constraints", lang_water, Y, N, PassKick::NONE, Y, N);
    known_run("Langevin constraints, Andersen", run_of(Loop::LANGEVIN, Y, Y, N, N, Y), Y, N, PassKick::NONE, N, N);
    known_run("Langevin bonded + PME", lang_protein, Y, N, PassKick::GCV, Y, Y);
    known_run("Langevin bonded + PME, FUSE_GATHER_VV 0", run_of(Loop::LANGEVIN, N, N, Y, Y, Y, Y, N), Y, N, PassKick::GCV, N, N);
    known_run("Langevin bonded only", run_of(Loop::LANGEVIN, N, N, Y, N, Y), Y, N, PassKick::NONE, N, N);
    const RunPlan stepwise = run_of(Loop::STEPWISE, N, N, N, N, Y);
    const RunPlan stepwise_single = run_of(Loop::STEPWISE, N, N, N, N, N);
    known_run("stepwise", stepwise, Y, Y, PassKick::NONE, N, N);
    known_run("stepwise, single list", stepwise_single, Y, N, PassKick::NONE, N, N);
    const RunPlan outside = RunPlan{};      // the stage entry points outside any loop: the two-launch form
    known_run("no loop", outside, N, N, PassKick::NONE, N, N);

    // ---- when a measured check is read ---------------------------------------------------------------------------------------------------------
    CHECK(!resolve_due(fluid, 110, 110) && resolve_due(fluid, 111, 110), "VV: one step later");
    CHECK(!resolve_due(lang_fluid, 111, 110) && resolve_due(lang_fluid, 112, 110), "Langevin: two steps later");
    CHECK(resolve_due(run_of(Loop::LANGEVIN, Y, N, N, N, Y), 110, 110), "Langevin without checks in its launches: a check left by a run before is read at once");

    // ---- before the pass -------------------------------------------------------------------------------------------------------------------------
    //                                                                                      cm th step gcv measure
    known_request("VV first step", fluid, at(101, 0, 0, Y, N), N, N, Y, N, N);
    known_request("VV mid step, cm every step", fluid, at(105, 1, 0, Y, N), Y, N, Y, N, N);
    known_request("VV cm every 3: 105", fluid, at(105, 3, 0, Y, N), Y, N, Y, N, N);
    known_request("VV cm every 3: 106", fluid, at(106, 3, 0, Y, N), N, N, Y, N, N);
    known_request("VV the step before a cadence step", fluid, at(109, 0, 0, Y, N), N, N, Y, N, Y);
    known_request("VV … with a check already issued", fluid, at(109, 0, 0, Y, Y), N, N, Y, N, N);
    known_request("VV … with lists that cannot be checked", fluid, at(109, 0, 0, N, N), N, N, Y, N, N);
    known_request("VV cadence step, dual list", fluid, at(110, 0, 0, Y, N), N, N, Y, N, N);
    known_request("VV last step", fluid, at(160, 1, 0, Y, N), Y, N, N, N, N);
    {
        StepShape s = at(159, 0, 0, Y, N); s.last = true;      // a run that ends right before a cadence step measures nothing
        known_request("VV last step before a cadence step", fluid, s, N, N, N, N, N);
    }
    known_request("VV thermostat every step", fluid, at(105, 1, 1, Y, N), Y, Y, N, N, N);
    known_request("VV thermostat every 3: 105", fluid, at(105, 0, 3, Y, N), N, Y, N, N, N);
    known_request("VV thermostat every 3: 106", fluid, at(106, 0, 3, Y, N), N, N, Y, N, N);
    known_request("VV thermostat step before a cadence step", fluid, at(109, 0, 1, Y, N), N, Y, N, N, Y);
    known_request("VV constraints", water, at(109, 1, 0, Y, N), Y, N, N, N, Y);
    known_request("VV bonded + PME, mid", protein, at(105, 0, 0, Y, N), N, N, N, Y, N);
    known_request("VV bonded + PME, cadence step, dual list", protein, at(110, 0, 0, Y, N), N, N, N, Y, N);
    known_request("VV bonded + PME, cadence step, single list", protein_single, at(110, 0, 0, N, N), N, N, N, N, N);
    known_request("VV bonded + PME, single list, off the cadence", protein_single, at(111, 0, 0, N, N), N, N, N, Y, N);
    known_request("VV bonded + PME, last", protein, at(160, 0, 0, Y, N), N, N, N, N, N);
    known_request("VV Andersen", andersen, at(109, 1, 0, Y, N), Y, N, N, N, N);
    known_request("Langevin fluid, mid", lang_fluid, at(105, 1, 0, Y, N), Y, N, Y, N, N);
    known_request("Langevin fluid, the step before a cadence step", lang_fluid, at(109, 0, 0, Y, N), N, N, Y, N, N);
    known_request("Langevin fluid, cadence step", lang_fluid, at(110, 0, 0, Y, N), N, N, Y, N, Y);
    known_request("Langevin fluid, cadence step, check issued", lang_fluid, at(110, 0, 0, Y, Y), N, N, Y, N, N);
    known_request("Langevin fluid, last step (a cadence step)", lang_fluid, at(160, 0, 0, Y, N), N, N, Y, N, Y);
    known_request("Langevin ignores a thermostat", lang_fluid, at(105, 0, 1, Y, N), N, N, Y, N, N);
    known_request("Langevin constraints, cadence step", lang_water, at(110, 3, 0, Y, N), N, N, N, N, Y);
    known_request("Langevin bonded + PME", lang_protein, at(110, 1, 0, Y, N), Y, N, N, Y, Y);
    known_request("stepwise", stepwise, at(109, 1, 0, Y, N), Y, N, N, N, N);
    {
        const StepRequest q = fused_halo_request(true, true);
        ++n_known;
        CHECK(q.cm && q.step && q.measure && !q.gcv && !q.th, "the fused ghosted step");
    }

    // ---- behind the pass -------------------------------------------------------------------------------------------------------------------------
    // 27 000 atoms: 106 blocks by either rule.                     form                     mode cm last meas at   nb   dest                  flip rep refresh
    known_stage("k_vv_mid", fluid, at(105, 0, 0, Y, N),            {StageForm::VV_MID,       -1, N, N, N, 0,   106, CmDest::NONE,          N, N, N});
    known_stage("k_vv_mid, first step", fluid, at(101, 1, 0, Y, N), {StageForm::VV_MID,      -1, Y, N, N, 0,   106, CmDest::ENGINE_HALF,   Y, Y, N});
    known_stage("k_vv_mid, cm + measure", fluid, at(109, 1, 0, Y, N), {StageForm::VV_MID,    -1, Y, N, Y, 110, 106, CmDest::ENGINE_HALF,   Y, Y, N});
    known_stage("k_vv_mid, check already issued", fluid, at(109, 3, 0, Y, Y), {StageForm::VV_MID, -1, N, N, N, 0, 106, CmDest::NONE,       N, N, N});
    known_stage("k_vv_mid, cadence step, dual", fluid, at(110, 0, 0, Y, N), {StageForm::VV_MID, -1, N, N, N, 0, 106, CmDest::NONE,         N, N, N});
    known_stage("k_vv_mid, cadence step, single list", fluid_single, at(110, 0, 0, N, N), {StageForm::VV_MID, -1, N, N, N, 0, 106, CmDest::NONE, N, N, Y});
    known_stage("k_vv_mid, last", fluid, at(160, 1, 0, Y, N),      {StageForm::VV_MID,       -1, Y, Y, N, 0,   106, CmDest::ENGINE_HALF,   Y, Y, N});
    known_stage("k_vv_mid, last, caller parts", fluid, at(160, 1, 0, Y, N, 27000, 7), {StageForm::VV_MID, -1, Y, Y, N, 0, 7, CmDest::CALLER, N, N, N});
    known_stage("k_vv_mid, last without cm, caller parts", fluid, at(160, 3, 0, Y, N, 27000, 7), {StageForm::VV_MID, -1, N, Y, N, 0, 106, CmDest::NONE, N, N, N});
    known_stage("k_vv_mid, mid-run, caller parts", fluid, at(105, 1, 0, Y, N, 27000, 7), {StageForm::VV_MID, -1, Y, N, N, 0, 106, CmDest::ENGINE_HALF, Y, Y, N});
    known_stage("k_vv_mid, 1M atoms", fluid, at(105, 1, 0, Y, N, 1048576), {StageForm::VV_MID, -1, Y, N, N, 0, 512, CmDest::ENGINE_HALF,   Y, Y, N});
    known_stage("k_vv_mid, 524 289 atoms", fluid, at(105, 1, 0, Y, N, 524289), {StageForm::VV_MID, -1, Y, N, N, 0, 256, CmDest::ENGINE_HALF, Y, Y, N});
    known_stage("k_con_step 1", water, at(109, 1, 0, Y, N),        {StageForm::CON_STEP,      1, Y, N, Y, 110, 33,  CmDest::ENGINE_HALF,   Y, Y, N});
    known_stage("k_con_step 2", water, at(160, 0, 0, Y, N),        {StageForm::CON_STEP,      2, N, Y, N, 0,   33,  CmDest::NONE,          N, N, N});
    known_stage("close + open", fluid, at(109, 1, 1, Y, N),        {StageForm::THERMO,       -1, Y, N, Y, 110, 106, CmDest::ENGINE_HALF,   N, N, N});
    known_stage("close + open, no cm", fluid, at(105, 0, 3, Y, N), {StageForm::THERMO,       -1, N, N, N, 0,   106, CmDest::NONE,          N, N, N});
    known_stage("close + scale: last step on a thermostat step", fluid, at(160, 1, 1, Y, N), {StageForm::THERMO_LAST, -1, Y, Y, N, 0, 106, CmDest::ENGINE_HALF, N, N, N});
    known_stage("last step off a thermostat step", fluid, at(160, 0, 3, Y, N), {StageForm::VV_MID, -1, N, Y, N, 0, 106, CmDest::NONE,      N, N, N});
    known_stage("close + open with constraints", water, at(105, 1, 1, Y, N), {StageForm::THERMO, 2, Y, N, N, 0, 33, CmDest::ENGINE_HALF,   N, N, N});
    known_stage("close + scale with constraints", water, at(160, 0, 1, Y, N), {StageForm::THERMO_LAST, 2, N, Y, N, 0, 33, CmDest::NONE,    N, N, N});
    known_stage("k_vv2", andersen, at(105, 1, 0, Y, N),            {StageForm::VV2,          -1, Y, Y, N, 0,   106, CmDest::ENGINE_FIRST,  N, Y, N});
    known_stage("k_vv2 without cm", outside, at(105, 0, 0, N, N),  {StageForm::VV2,          -1, N, Y, N, 0,   106, CmDest::NONE,          N, N, N});
    known_stage("k_vv2, caller parts", outside, at(105, 1, 0, N, N, 27000, 7), {StageForm::VV2, -1, Y, Y, N, 0, 7,  CmDest::CALLER,        N, N, N});
    known_stage("k_vv2, 524 289 atoms", outside, at(105, 1, 0, N, N, 524289), {StageForm::VV2, -1, Y, Y, N, 0, 1024, CmDest::ENGINE_FIRST, N, Y, N});
    known_stage("k_vv2, cadence step, single list", run_of(Loop::VV, Y, N, N, N, N), at(110, 0, 0, N, N), {StageForm::VV2, -1, N, Y, N, 0, 106, CmDest::NONE, N, N, Y});
    known_stage("launch_langevin", lang_fluid, at(105, 1, 0, Y, N), {StageForm::LANGEVIN,    -1, Y, N, N, 0,   106, CmDest::ENGINE_HALF,   Y, Y, N});
    known_stage("launch_langevin, cadence step: never measures", lang_fluid, at(110, 0, 0, Y, N), {StageForm::LANGEVIN, -1, N, N, N, 0, 106, CmDest::NONE, N, N, Y});
    known_stage("launch_langevin, 524 289 atoms", lang_fluid, at(105, 0, 0, Y, N, 524289), {StageForm::LANGEVIN, -1, N, N, N, 0, 1024, CmDest::NONE, N, N, N});
    known_stage("k_con_step 3", lang_water, at(110, 1, 0, Y, N),   {StageForm::CON_STEP,      3, Y, N, Y, 110, 33,  CmDest::ENGINE_HALF,   Y, Y, Y});
    known_stage("k_con_step 3, last step", lang_water, at(160, 3, 0, Y, Y), {StageForm::CON_STEP, 3, N, N, N, 0, 33, CmDest::NONE,         N, N, Y});
    {
        StepShape solo = at(105, 1, 0, N, N), peers = solo, end = at(160, 1, 0, N, N, 27000, 7), big = at(105, 0, 0, N, N, 1048576), big_peers = big;
        peers.solo = N; big_peers.solo = N;
        known_stage("stepwise, solo", stepwise, solo,              {StageForm::VV_MID,       -1, Y, N, N, 0,   106, CmDest::ENGINE_HALF,   Y, N, N});
        known_stage("stepwise, peers", stepwise, peers,            {StageForm::VV_MID,       -1, Y, N, N, 0,   106, CmDest::ENGINE_FIRST,  N, N, N});
        known_stage("stepwise, stop with cm", stepwise, end,       {StageForm::VV_MID,       -1, Y, Y, N, 0,   7,   CmDest::CALLER,        N, N, N});
        known_stage("stepwise, solo, no cm: the halves still alternate", stepwise, big, {StageForm::VV_MID, -1, N, N, N, 0, 512, CmDest::NONE, Y, N, N});
        known_stage("stepwise, peers, 1M atoms", stepwise, big_peers, {StageForm::VV_MID,    -1, N, N, N, 0,   1024, CmDest::NONE,         N, N, N});
        StepShape cadence = at(110, 0, 0, N, N);
        known_stage("stepwise, cadence step, single list", stepwise_single, cadence, {StageForm::VV_MID, -1, N, N, N, 0, 106, CmDest::NONE, Y, N, Y});
        known_stage("stepwise, cadence step, dual list", stepwise, cadence, {StageForm::VV_MID, -1, N, N, N, 0, 106, CmDest::NONE,         Y, N, N});
    }
    // the pass integrated: nothing to launch
    known_plan("integrated", plan_stage(fluid, at(105, 1, 0, Y, N), plan_request(fluid, at(105, 1, 0, Y, N)), true), {StageForm::NONE, -1, N, N, N, 0, 0, CmDest::NONE, N, N, N});
    known_plan("integrated, Langevin cadence step", plan_stage(lang_fluid, at(110, 1, 0, Y, N), plan_request(lang_fluid, at(110, 1, 0, Y, N)), true), {StageForm::NONE, -1, N, N, N, 0, 0, CmDest::NONE, N, N, Y});
    // ---- the opening launch ----------------------------------------------------------------------------------------------------------------------
    known_plan("k_vv1", plan_open(fluid, at(100, 1, 0, Y, N), 60), {StageForm::VV1, -1, N, N, N, 0, 106, CmDest::NONE, N, N, N});
    known_plan("k_vv1, 524 289 atoms", plan_open(outside, at(100, 0, 0, N, N, 524289)), {StageForm::VV1, -1, N, N, N, 0, 1024, CmDest::NONE, N, N, N});
    known_plan("k_con_step 0", plan_open(water, at(100, 1, 0, Y, N), 60), {StageForm::CON_STEP, 0, N, N, N, 0, 33, CmDest::NONE, N, N, N});
    known_plan("a run of no steps", plan_open(fluid, at(100, 1, 0, Y, N), 0), {StageForm::NONE, -1, N, N, N, 0, 0, CmDest::NONE, N, N, N});
    known_plan("Langevin opens nothing", plan_open(lang_fluid, at(100, 1, 0, Y, N), 60), {StageForm::NONE, -1, N, N, N, 0, 0, CmDest::NONE, N, N, N});
}

// Preconditions the admit table (admit.h) and the entry points enforce — stated here, skipped, not asserted:
//   no Andersen coupling next to constraints, sites or a rescaling thermostat; no partial buffer of the caller's next to constraints or sites (mhip_domain_run refuses them);
//   the two-launch form is handed a partial buffer only on a step that removes the centre-of-mass motion (mhip_vv_halo_end_parts); a stepwise step that stops with cm has one
static bool precondition(const RunShape& rs, const RunPlan& r, const StepShape& s) {
    if (rs.andersen && (rs.items || s.thermo_every > 0)) return false;
    if (rs.items && s.n_parts_last > 0) return false;
    if (rs.items && rs.loop == Loop::STEPWISE) return false;
    if (rs.loop == Loop::VV && !r.fused && s.n_parts_last > 0 && !step_cm(s)) return false;
    if (rs.loop == Loop::STEPWISE && step_cm(s) && s.last && s.n_parts_last == 0) return false;
    return true;
}

static void sweep() {
    const Loop loops[] = {Loop::VV, Loop::LANGEVIN, Loop::STEPWISE};
    // first + 1, mid, cadence − 1, cadence, last on a cadence step, last off it
    struct Pos { int64_t step; bool last; };
    const Pos positions[] = {{102, false}, {105, false}, {109, false}, {110, false}, {160, true}, {157, true}};
    const int64_t atoms[] = {1, 255, 256, 257, 65536, 65537, 261888, 262144, 262145, 524289, 526336, 1048575, 1048576, (int64_t)1 << 30};
    const int cm_every[] = {0, 1, 3}, th_every[] = {0, 1, 3}, parts[] = {0, 7};      // (no block rule gives 7 blocks for these atom counts, and the items get 33)
    long long n = 0, skipped = 0;
    for (Loop loop : loops) for (int bits = 0; bits < 128; ++bits) {
        RunShape rs;
        rs.loop = loop; rs.andersen = bits & 1; rs.items = bits & 2; rs.bonded = bits & 4; rs.pme = bits & 8; rs.dual = bits & 16; rs.fuse_step = bits & 32; rs.fuse_gcv = bits & 64;
        const RunPlan r = plan_run(rs);
        CHECK(!(r.kick != PassKick::NONE && rs.items), "a force launch integrates next to work items");
        CHECK(!r.async || r.fused, "checks inside the launches of the two-launch form");
        for (const Pos& pos : positions) for (int sb = 0; sb < 8; ++sb) for (int ce : cm_every) for (int te : th_every) for (int np : parts) for (int64_t na : atoms) {
            StepShape s;
            s.step = pos.step; s.last = pos.last; s.remove_cm_every = ce; s.thermo_every = te; s.due = pos.step % EVERY == 0; s.due_next = (pos.step + 1) % EVERY == 0;
            s.async_ok = sb & 1; s.trk_issued = sb & 2; s.solo = sb & 4; s.n_atoms = na; s.item_blocks = 33; s.n_parts_last = np;
            ++n;
            if (!precondition(rs, r, s)) { ++skipped; continue; }
            const StepRequest q = plan_request(r, s);
            const bool vv = loop == Loop::VV, lang = loop == Loop::LANGEVIN;
            CHECK(!(q.step && q.gcv), "both kinds of integrating pass asked for");
            if (vv && (s.last || rs.items || q.th || !r.fused)) CHECK(!q.step && !q.gcv, "VV asks a pass to integrate: last %d items %d th %d fused %d", (int)s.last, (int)rs.items, (int)q.th, (int)r.fused);
            if (!lang) CHECK(q.cm == (ce != 0 && s.step % ce == 0), "cm");
            if (q.measure) CHECK(r.async && s.async_ok && !s.trk_issued && (lang ? s.due : (s.due_next && !s.last)), "measure asked: loop %d step %lld", (int)loop, (long long)s.step);
            // the pass integrated: nothing is asked
            const StagePlan none = plan_stage(r, s, q, true);
            CHECK(none.form == StageForm::NONE && none.nb == 0 && !none.measure && none.dest == CmDest::NONE && !none.flip && !none.repend, "a stage planned behind a pass that integrated");
            const StagePlan p = plan_stage(r, s, q, false);
            CHECK(p.form != StageForm::NONE && p.form != StageForm::VV1, "no closing form");
            CHECK(p.nb >= 1, "%d blocks", p.nb);
            const bool engine_dest = p.dest == CmDest::ENGINE_HALF || p.dest == CmDest::ENGINE_FIRST;
            if (engine_dest) CHECK(p.nb <= CM_HALF_PARTS, "%d partials into a half of %d", p.nb, CM_HALF_PARTS);
            CHECK((p.nb == s.n_parts_last) == (p.dest == CmDest::CALLER), "nb %d, caller parts %d, dest %d", p.nb, s.n_parts_last, (int)p.dest);
            CHECK((p.dest != CmDest::NONE) == q.cm, "a destination without cm, or cm without one");
            if (p.measure) CHECK(r.async && s.async_ok && !s.trk_issued && (lang ? (q.measure && p.check_step == s.step) : (s.due_next && !s.last && p.check_step == s.step + 1)), "stage measures: loop %d", (int)loop);
            if (p.measure) CHECK(p.form != StageForm::LANGEVIN && p.form != StageForm::VV2 && p.form != StageForm::THERMO_LAST, "form %d cannot measure", (int)p.form);
            CHECK(p.repend == (loop != Loop::STEPWISE && q.cm && engine_dest && !q.th), "pending Σ m v: repend %d cm %d dest %d th %d", (int)p.repend, (int)q.cm, (int)p.dest, (int)q.th);
            if (p.flip) CHECK(p.dest != CmDest::ENGINE_FIRST && p.dest != CmDest::CALLER, "the halves turn under a launch that does not write one");
            if (loop != Loop::STEPWISE) CHECK(p.flip == (p.repend && p.dest == CmDest::ENGINE_HALF), "flip %d repend %d", (int)p.flip, (int)p.repend);
            CHECK((p.con_mode >= 0) == (rs.items && p.form != StageForm::VV2), "k_con_step without items, or items without it");
            if (p.form == StageForm::CON_STEP) CHECK(p.con_mode == (lang ? 3 : s.last ? 2 : 1), "mode %d", p.con_mode);
            if (p.form == StageForm::THERMO || p.form == StageForm::THERMO_LAST) CHECK(q.th && (p.form == StageForm::THERMO_LAST) == s.last && (p.con_mode == 2 || p.con_mode == -1), "thermostat form");
            if (q.th) CHECK(p.form == StageForm::THERMO || p.form == StageForm::THERMO_LAST, "a thermostat step closed by form %d", (int)p.form);
            CHECK(p.refresh_behind == (!r.pre && s.due), "refresh");
        }
    }
    std::printf("sweep: %lld step shapes (%lld outside the preconditions)\n", n, skipped);
}

int main() {
    known_answers();
    std::printf("known answers: %d\n", n_known);
    sweep();
    std::printf(failures ? "%d FAILURES\n" : "step_plan_check: all passed\n", failures);
    return failures ? 1 : 0;
}
