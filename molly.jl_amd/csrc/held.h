// held.h — what the context currently holds, and which call voids which part of it.  Host-only: fifteen booleans and the events that
// change them; no device code, nothing of the engine (tests/host/held_check.cpp runs it alone).
//
// The engine reads the flags through the accessors and the queries at the end; it changes them ONLY through the events below, one
// per thing that can happen to a context.  This table is the rule (DESIGN.md §5a repeats it):  1 / 0 = set / cleared,  · = untouched.
//
//                             stale moved xsrch inner outrn frc  total fprev state param spend vchk  trk  plate intr
//   atoms_replaced(false)       1     ·     ·     ·     ·    0     ·     ·     ·     ·     ·     ·    0     ·     ·     set_atom_counts
//   atoms_replaced(true)        1     0     ·     ·     ·    0     0     ·     ·     ·     0     ·    0     ·     0     the commit of device_replan
//   interactions_changing()     ·     ·     ·     ·     ·    ·     0     0     ·     ·     ·     ·    ·     ·     ·     set_atoms, set_exceptions: on entry
//   params_changed(fmt)        fmt    ·     ·     ·     ·    0     ·     ·     ·     1     ·     ·    ·     ·     ·     set_atoms: done (fmt: the lists are in the other entry format)
//   exceptions_changed()        1     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     ·    ·     ·     ·     set_exceptions: done
//   terms_changed()             ·     ·     ·     ·     ·    ·     0     ·     ·     ·     ·     ·    ·     ·     ·     set_bonds / angles / torsions / ewald_exclusions / virtual_sites, set_pme on entry
//   pme_changed()               ·     ·     ·     ·     ·    0     ·     ·     ·     ·     ·     ·    ·     ·     ·     set_pme: done
//   lists_voided()              1     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     ·    ·     ·     ·     a new launch shape or cell grid, set_ghost_margin, lists outrun by a set_state
//   box_changed(false)          1     ·     ·     ·     ·    0     ·     ·     0     ·     ·     ·    ·     ·     ·     set_triclinic
//   box_changed(true)           1     ·     ·     ·     ·    0     0     0     0     ·     ·     ·    ·     ·     ·     set_box (a live context)
//   state_write_begins()        ·     ·     ·     ·     ·    ·     ·    (a)    ·     ·     1     ·    ·     ·     ·     set_state, place_virtual_sites: before the write
//   coords_written(skin)       (b)   (b)    ·     ·     ·    0     ·     ·     1     ·     ·     ·    ·     ·     ·     set_state with coordinates, place_virtual_sites
//   state_compared(dx, dv)      ·    (c)    ·     ·     ·   (c)    ·     0     ·     ·     0     ·   (c)    ·     ·     the read-back in lists_after_set_state
//   moved_coords_taken(…)       ·     0     ·     ·     ·    ·     ·     ·     ·     ·     ·    (d)   ·     ·     ·     lists_after_set_state, behind the read-back
//   export_wants_search()       ·     ·     1     ·     ·    ·     ·     ·     ·     ·     ·     ·    ·     ·     ·     … a single list that covers the moved coordinates, but is not theirs
//   vel_check_taken()           ·     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     0    ·     ·     ·     start_lists, ensure_built
//   lists_searched(dual)        0     0     0    (e)   (e)   ·     0     ·     ·     ·     ·     ·    ·     ·     ·     the end of rebuild_impl
//   inner_list_made(how)        ·     ·     ·     1    (f)   ·     ·     ·     ·     ·     ·     ·    ·    (f)    ·     finish_prune, adopt_outer_list
//   prune_wanted()              ·     ·     ·     0     ·    ·     ·     ·     ·     ·     ·     ·    ·     ·     ·     the policy's PRUNE, request_prune, a grown inner skin
//   outrun_taken()              ·     ·     ·     ·     0    ·     ·     ·     ·     ·     ·     ·    ·     ·     ·     after_forces
//   prune_read()                ·     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     ·    ·     0     ·     prune_resolve
//   forces_total()              ·     ·     ·     ·     ·    1     ·     ·     ·     ·     ·     ·    ·     ·     ·     the end of step_forces
//   forces_partial()            ·     ·     ·     ·     ·    0     ·     ·     ·     ·     ·     ·    ·     ·     ·     forces, specific_forces, general_forces, tune_launch
//   drifted()                   ·     ·     ·     ·     ·    0     ·     ·     ·     ·     ·     ·    ·     ·     ·     every integrator launch that moves the coordinates on
//   run_begins()                ·     ·     ·     ·     ·    ·     0     ·     ·     ·     ·     ·    ·     ·     ·     vv_init
//   run_ended(total)            ·     ·     ·     ·     ·    ·   total   ·     ·     ·     ·     ·    ·     ·     ·     the last step of vv_loop
//   check_issued()              ·     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     ·    1     ·     ·     issue_track
//   check_read()                ·     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     ·    0     ·     ·     resolve_track
//   interior_pass(ran)          ·     ·     ·     ·     ·    ·     ·     ·     ·     ·     ·     ·    ·     ·    ran    halo_interior; step_forces (false: the rest has run)
//
//   (a) fprev = frc, if no comparison was pending yet (the first write since the last read-back decides)
//   (b) lists with a skin that are not stale: moved = 1 (their displacement is measured at the next use); else stale = 1
//   (c) the same coordinates again (!dx): moved = 0, and frc = 1 if fprev and not stale;  dx or dv: trk = 0
//   (d) new velocities on lists that live on: vchk = 1
//   (e) a dual list: inner = 0, outrn = 0;  a single list leaves both
//   (f) READ_NOW: plate = 0, outrn = the verdict read;  READ_LATE: plate = 1, outrn = 0;  ADOPTED: outrn = 0
//
// What the engine relies on (swept over every state × every event by the host check):
//   1. after lists_searched(): not stale, no moved coordinates pending, no export search pending, no run-total force
//   2. frc is turned on by forces_total() alone, and by state_compared(false, ·) when the forces were current before the write and
//      the lists are not stale; frc_run_total by run_ended(true) alone; stale is cleared by lists_searched() alone; inner is set by
//      inner_list_made() alone; trk by check_issued() alone; plate by inner_list_made(READ_LATE) alone; intr by interior_pass(true) alone
//   3. after atoms_replaced, exceptions_changed, lists_voided, box_changed, params_changed(true): stale — hence no run forces to
//      reuse, no inner list that stands, no check that applies
//   4. after coords_written(): frc off, the coordinates set, and stale or moved — no force survives a write that is not compared
//   5. reusable_run_forces() implies frc, frc_run_total, not stale, not moved
//   6. params is never cleared; state is cleared by box_changed() alone
//   7. fprev is turned on by state_write_begins() alone, and only by the first write since the last read-back, when frc was on
#pragma once

namespace mhip {

class Held {
    bool stale_ = true;                  // no pair list of the atoms, the box and the exceptions as they now are
    bool coords_moved_ = false;          // coordinates came in that the lists (with a skin) have not been measured against yet
    bool export_needs_search_ = false;   // a single list covers the moved coordinates for forces; mhip_export_neighbors wants the list of NOW
    bool inner_valid_ = false;           // the inner list of the dual scheme holds every pair within the cutoffs
    bool prune_disp_exceeded_ = false;   // the last prune found the outer list outrun: search again and redo the pass
    bool frc_valid_ = false;             // frc[cur] (+ the side array) is the total force of the coordinates held
    bool frc_run_total_ = false;         // … left in frc[cur] alone, in the current order, by the last step of a run
    bool frc_before_set_state_ = false;  // were the forces current when the (possibly identical) coordinates came in?
    bool state_set_ = false;             // coordinates have been handed over (for the box as it is)
    bool params_set_ = false;            // per-atom parameters have been handed over
    bool state_pending_ = false;         // a state was written whose comparison with the state before has not been read back
    bool vel_check_due_ = false;         // velocities were replaced since the last validity check of the lists
    bool trk_issued_ = false;            // a list check measured by an integrator launch is in flight
    bool prune_pending_ = false;         // the figures of a pruning pass wait behind an event (read late)
    bool interior_done_ = false;         // halo_interior ran the blocks without ghosts: the next step_forces runs the rest

  public:
    // ---- the flags, read-only ------------------------------------------------------------------------------------------------------
    bool stale() const { return stale_; }
    bool coords_moved() const { return coords_moved_; }
    bool export_needs_search() const { return export_needs_search_; }
    bool inner_valid() const { return inner_valid_; }
    bool prune_disp_exceeded() const { return prune_disp_exceeded_; }
    bool frc_valid() const { return frc_valid_; }
    bool frc_run_total() const { return frc_run_total_; }
    bool frc_before_set_state() const { return frc_before_set_state_; }
    bool state_set() const { return state_set_; }
    bool params_set() const { return params_set_; }
    bool state_pending() const { return state_pending_; }
    bool vel_check_due() const { return vel_check_due_; }
    bool trk_issued() const { return trk_issued_; }
    bool prune_pending() const { return prune_pending_; }
    bool interior_done() const { return interior_done_; }

    // ---- the events ------------------------------------------------------------------------------------------------------------------
    // a new local atom set in its identity order.  in_engine: made by the re-plan inside a step (device_replan), which also has no
    // set_state comparison, interior pass or run forces to carry over
    void atoms_replaced(bool in_engine) {
        stale_ = true; frc_valid_ = false; trk_issued_ = false;
        if (in_engine) { interior_done_ = false; frc_run_total_ = false; coords_moved_ = false; state_pending_ = false; }
    }
    // new charges / σ / ϵ / masses / exceptions are on their way in: neither a finished run's forces nor those held before a set_state stand
    void interactions_changing() { frc_run_total_ = false; frc_before_set_state_ = false; }
    void params_changed(bool entry_format_changed) {
        if (entry_format_changed) stale_ = true;   // the lists in use are in the other entry format
        params_set_ = true; frc_valid_ = false;
    }
    void exceptions_changed() { stale_ = true; }   // ≙ cache invalidation after append_excluded_pairs! (test/gpu_consistency.jl:494-527)
    // (new terms change the total force: what a finished run left in frc[cur] is not the next run's first force any more)
    void terms_changed() { frc_run_total_ = false; }
    void pme_changed() { frc_valid_ = false; }
    // a new launch shape, cell grid or ghost margin: every list is void
    void lists_voided() { stale_ = true; }
    // from here on, whichever way the call ends: no list, no forces, the coordinates to be handed over again.  live: the box of a
    // live context (set_box), which may hold a finished run's forces and a set_state not yet compared
    void box_changed(bool live) {
        stale_ = true; frc_valid_ = false; state_set_ = false;
        if (live) { frc_run_total_ = false; frc_before_set_state_ = false; }
    }
    // a state is about to be written over the one held.  true: no comparison was pending, the words the write raises start from zero
    bool state_write_begins() {
        const bool first = !state_pending_;
        if (first) frc_before_set_state_ = frc_valid_;
        state_pending_ = true;
        return first;
    }
    // New coordinates, same atoms: the sorted order, the tiles and the pair lists stay (≙ the reference's GPU path, which re-reads
    // moved coordinates at every call and redoes its sort / tile search only at the step cadence, ext/MollyCUDAExt.jl:774-783).
    // Whether the lists still cover every cutoff sphere is decided by displacement at the next force call (lists_after_set_state);
    // lists that have no skin to spend are rebuilt at once.
    void coords_written(bool lists_have_skin) {
        if (!stale_ && lists_have_skin) coords_moved_ = true; else stale_ = true;
        frc_valid_ = false; state_set_ = true;
    }
    // what did the write really change?  (a state handed back as it was — a run continued in chunks — changes nothing)
    void state_compared(bool coords_differ, bool vel_differ) {
        state_pending_ = false;
        if (!coords_differ) { coords_moved_ = false; if (frc_before_set_state_ && !stale_) frc_valid_ = true; }   // the same coordinates again: what was computed for them stands
        frc_before_set_state_ = false;
        if (coords_differ || vel_differ) trk_issued_ = false;      // a measurement in flight describes the state that was replaced
    }
    // behind the read-back: true when the lists have to be measured against moved coordinates now.
    // New velocities on old coordinates (re-thermalisation, a temperature ramp, a replica-exchange swap): the inner skin was sized
    // for the speeds of the run before.  Look at the new ones at the start of the next run instead of at the next cadence step.
    bool moved_coords_taken(bool vel_new, bool lists_have_skin) {
        if (vel_new && !stale_ && lists_have_skin && !coords_moved_) vel_check_due_ = true;
        if (!coords_moved_) return false;
        coords_moved_ = false;
        if (stale_) return false;
        vel_check_due_ = vel_check_due_ || vel_new;
        return true;
    }
    void export_wants_search() { export_needs_search_ = true; }
    void vel_check_taken() { vel_check_due_ = false; }
    // the outer (or only) list was searched at the coordinates held; the sort moved the atoms
    void lists_searched(bool dual) {
        if (dual) { inner_valid_ = false; prune_disp_exceeded_ = false; }   // the next force pass prunes the outer list into the inner one
        stale_ = false; coords_moved_ = false; export_needs_search_ = false;
        frc_run_total_ = false;
    }
    // READ_NOW: the pruning pass's figures were read at once, outer_outrun is their verdict; READ_LATE: they wait behind an event; ADOPTED: the outer list stands in
    enum class Prune { READ_NOW, READ_LATE, ADOPTED };
    void inner_list_made(Prune how, bool outer_outrun = false) {
        inner_valid_ = true;
        if (how == Prune::READ_NOW) { prune_pending_ = false; prune_disp_exceeded_ = outer_outrun; }
        else if (how == Prune::READ_LATE) { prune_pending_ = true; prune_disp_exceeded_ = false; }
        else prune_disp_exceeded_ = false;
    }
    void prune_wanted() { inner_valid_ = false; }   // the next force pass re-prunes the outer list at the then-current coordinates
    void outrun_taken() { prune_disp_exceeded_ = false; }
    void prune_read() { prune_pending_ = false; }
    void forces_total() { frc_valid_ = true; }
    void forces_partial() { frc_valid_ = false; }   // frc[cur] holds one kind of term only
    void drifted() { frc_valid_ = false; }          // frc[cur] belongs to the coordinates before the drift
    void run_begins() { frc_run_total_ = false; }
    void run_ended(bool total_in_place) { frc_run_total_ = total_in_place; }   // (side arrays are added by the kick, not folded)
    void check_issued() { trk_issued_ = true; }
    void check_read() { trk_issued_ = false; }
    void interior_pass(bool ran) { interior_done_ = ran; }

    // ---- the queries -----------------------------------------------------------------------------------------------------------------
    // frc[cur] holds the TOTAL force of the coordinates the engine holds, in the current order (left there by the last step of a run
    // that had no side arrays pending).  A run that continues from exactly that state — the chunked simulate! of test/simulation.jl:16-57,
    // a benchmark's consecutive windows — finds the forces of its first step already there: the reference recomputes them
    // (simulators.jl:564-571), which yields the same numbers from the same lists in the same order.
    bool reusable_run_forces() const { return frc_run_total_ && frc_valid_ && !stale_ && !coords_moved_; }
    // a searched outer list with a valid inner list: what a check in flight measured, a late prune read-back describes, and the
    // launches that measure checks on the way walk.  False: the lists have been replaced meanwhile
    bool inner_list_stands() const { return !stale_ && inner_valid_; }
    // may the blocks without ghosts run ahead of the ghost exchange?  Only over lists that are known to be good
    bool split_pass_ok(bool dual, bool lazy_single) const { return dual ? inner_valid_ : !lazy_single; }

    // ---- for the host check: the state as a bit vector, in the order of the table's columns ----------------------------------------
    static constexpr int N_FLAGS = 15;
    unsigned bits() const {
        const bool f[N_FLAGS] = {stale_, coords_moved_, export_needs_search_, inner_valid_, prune_disp_exceeded_, frc_valid_, frc_run_total_, frc_before_set_state_,
                                 state_set_, params_set_, state_pending_, vel_check_due_, trk_issued_, prune_pending_, interior_done_};
        unsigned b = 0;
        for (int k = 0; k < N_FLAGS; ++k) b |= (f[k] ? 1u : 0u) << k;
        return b;
    }
    static Held from_bits(unsigned b) {
        Held h;
        bool* const f[N_FLAGS] = {&h.stale_, &h.coords_moved_, &h.export_needs_search_, &h.inner_valid_, &h.prune_disp_exceeded_, &h.frc_valid_, &h.frc_run_total_, &h.frc_before_set_state_,
                                  &h.state_set_, &h.params_set_, &h.state_pending_, &h.vel_check_due_, &h.trk_issued_, &h.prune_pending_, &h.interior_done_};
        for (int k = 0; k < N_FLAGS; ++k) *f[k] = (b >> k) & 1u;
        return h;
    }
};

}  // namespace mhip
