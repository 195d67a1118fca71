// list_policy.h — when a pair list may live on, when the inner list is pruned again, when the outer list is searched again.
// Host-only arithmetic on a handful of doubles: no device code, nothing of the engine (tests/host/list_policy_check.cpp runs it alone).
//
// The lists: an OUTER list holds every pair within r_list + outer_margin of the coordinates at its search; the INNER list, pruned
// from it, every pair within rc_max + skin_in of the coordinates at its prune (skin_in <= skin = r_list − rc_max).  A list with a
// margin m still holds every pair it has to as long as nobody moved more than m / 2 since it was made: covered().  Without the dual
// list a single list of radius r_list is kept by the same test against skin ("lazy single").
//
// One decision, decide(), is made from one measurement in three call forms.  They differ only in WHEN the decision is applied,
// and every such difference is a column of this table (the constructors of Applied below are its rows):
//
//   form                           drift horizon               outer-test headroom (steps)   check-in accepted if      check-in allowed when
//   synchronous  (refresh)         every                       0                             k >= 3                    inside a run that owns its loop, no ghosts
//   asynchronous (resolve_track)   every                       step − measured step          k >= 3                    always (the caller owns the loop)
//   collective   (plan_decide)     every + max(late − 1, 0)    1 + late                      k >= 3 and k > late + 1   the caller gave a check_in pointer
//   lazy single  (refresh)         every                       (no outer list)               k >= 3                    inside a run that owns its loop
//
// The asynchronous and the collective form keep the look-again step differently: the engine's own loops read next_check_step,
// the collective caller is handed k and keeps the step itself.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace mhip {

struct ListPolicy {
    // ---- the constants of the rule -----------------------------------------------------------------------------------------------
    static constexpr double SLACK = 0.98;               // the share of a margin the tests spend (the rest: rounding of the fp32 displacements)
    static constexpr double CHECK_IN_SLACK = 0.49;      // … of which a displacement alone may use half: SLACK / 2
    static constexpr double EMPIRICAL_STRETCH = 1.5;    // no time step known: the displacement rate seen so far, times this
    static constexpr double GROWTH_MIN = 1.1, GROWTH_MAX = 3.0;      // how much the top speed is taken to grow over an interval: as it did over the last, clamped
    static constexpr double GROWTH_UNKNOWN = 1.25;      // … before there is a last one
    static constexpr double HEADROOM_STRETCH = 1.25;    // the outer test's headroom: the top speed, times this, over the steps until the prune runs
    static constexpr double SKIN_INTERVALS = 3.0;       // the inner skin covers the drift of this many check intervals
    static constexpr int MIN_CHECK_IN = 3;              // a look-again closer than this is not worth a check of its own
    static constexpr double SINGLE_PRUNE_SLOP = 0.02;   // nm: outer_margin <= 2·skin_in − skin + this leaves an outer list no second prune
    static constexpr int OUTRUN_WINDOW = 2, OUTRUN_LIMIT = 3;        // an outer list outrun within this many intervals of its search, this often: dual list off

    // ---- state ---------------------------------------------------------------------------------------------------------------------
    double skin = 0, rc_max = 0;                 // r_list − largest cutoff | the largest cutoff
    double skin_in = 0, skin_in_adapted = 0;     // the inner list's skin | as a run has grown it (a skin once grown stays grown)
    double outer_margin = 0;
    double cur_dt = 0;                           // the time step of the run in progress, 0 when driven from outside (no drift bound from speeds)
    double last_vmax = 0, prev_vmax = 0;         // the fastest owned atom at the last measurement | at the one before
    int64_t next_check_step = -1;                // a check between the cadence steps asked for by a look-again decision, −1: none
    int64_t last_prune_step = 0, last_outer_step = 0;
    int early_outer = 0;                         // outer lists outrun soon after their search, in a row
    bool want_margin_zero = false;               // the grown inner skin leaves the outer margin nothing to do: drop it at the next cadence step
    int64_t n_disp_checks = 0;                   // measurements taken
    bool inner_skin_fixed = false;               // the inner skin never grows (the owner's switch)

    // ---- the one slack test ------------------------------------------------------------------------------------------------------
    // a list with `margin` to spend, d of it used up by the farthest atom and `ahead` more expected: still good?  (NaN: no)
    static bool covered(double d, double ahead, double margin) { return 2.0 * (d + ahead) <= SLACK * margin; }
    // How far atoms may have moved since the outer search for a prune to be trustworthy: the outer list holds every pair within
    // r_list + outer_margin of then, the prune wants every pair within rc_max + skin_in of now.
    double prune_margin() const { return outer_margin + (skin - skin_in); }
    bool prune_stands(double d_outer) const { return covered(d_outer, 0.0, prune_margin()); }
    bool check_due(int64_t step, int every) const { return step % every == 0 || (next_check_step >= 0 && step >= next_check_step); }

    // the inner skin at the start: the owner's floor (or what a run grew it to) where the engine's own criteria prune, else all of skin
    void start_inner_skin(bool tight, double floor, bool grown_stays = true) {
        skin_in = tight ? std::min(skin, std::max(grown_stays ? skin_in_adapted : 0.0, floor)) : skin;
    }
    // a measurement came in: the speeds (the one before: as the caller remembers it, else the last one taken)
    void measured(double v_max) { measured(v_max, last_vmax); }
    void measured(double v_max, double v_before) { prev_vmax = v_before; last_vmax = v_max; ++n_disp_checks; }

    // Upper estimate of how much further anybody gets in `steps` more steps.  Inside a run the time step is known: the fastest
    // atom's speed now, stretched by how much the top speed grew since the last check (at least 10 %), times the interval.  Driven
    // from outside there is no time step: the displacement rate seen so far, times 1.5.
    double drift_ahead(double d_so_far, int64_t steps_so_far, int steps) const {
        if (!(cur_dt > 0)) return EMPIRICAL_STRETCH * d_so_far * (double)steps / (double)std::max<int64_t>(steps_so_far, 1);
        const double growth = prev_vmax > 0 ? std::min(std::max(last_vmax / prev_vmax, GROWTH_MIN), GROWTH_MAX) : GROWTH_UNKNOWN;
        return last_vmax * growth * cur_dt * steps;
    }
    // The inner list must outlive at least one check interval: if the fastest atoms cover more than a third of the inner skin between
    // two checks, the skin grows (up to the reference's own r_list − cutoff); the caller prunes afresh with the larger radius.
    // (Only for a dual list whose prunes the engine schedules: every caller of decide() sees to that before it asks.)
    bool grow_inner_skin(double drift_per_interval, bool ghosts) {
        if (!(skin_in < skin) || inner_skin_fixed) return false;
        const double need = std::min(skin, SKIN_INTERVALS * drift_per_interval / SLACK);
        if (need <= skin_in) return false;
        skin_in = need; skin_in_adapted = need;
        // An outer list serves a second prune only while nobody moved (outer_margin + skin − skin_in)/2 since its search, and the inner
        // list is not due before ≈ skin_in/2: with outer_margin <= 2·skin_in − skin every outer list is pruned exactly once, and its
        // margin only makes the search dearer.
        if (!ghosts && outer_margin > 0 && outer_margin <= 2.0 * skin_in - skin + SINGLE_PRUNE_SLOP) want_margin_zero = true;
        return true;
    }
    // A prune found its outer list outrun.  If that keeps happening before the outer list has paid for itself (fast light atoms,
    // small time step), the dual list is a loss: true = give it up.
    bool outer_outrun(int64_t step, int every) {
        if (step - last_outer_step <= OUTRUN_WINDOW * (int64_t)every) return ++early_outer >= OUTRUN_LIMIT;
        early_outer = 0;
        return false;
    }

    // ---- the decision --------------------------------------------------------------------------------------------------------------
    struct Measured {
        double d;           // largest displacement since the prune (single list: since its search); +inf: there is no inner list to vouch for
        double d_outer;     // … since the outer search
        int64_t steps;      // steps from the prune to the measurement
    };                      // (the speeds of the measurement: measured())
    struct Applied {        // when the decision is applied: see the table at the top
        int every = 0;
        int horizon = 0;                    // steps the drift is estimated over
        double headroom_steps = 0;          // steps from the measurement to the prune it may ask for
        int min_check_in = MIN_CHECK_IN;    // smallest look-again distance that is accepted
        bool check_in = false;              // a look-again may be asked for at all
        int64_t measured_at = 0;            // the measured step
        bool keeps_step = true;             // a look-again sets next_check_step (else: the caller keeps the step)
        bool single = false;                // the lazy single list
        bool ghosts = false;                // a ghosted sub-domain (it never drops its outer margin on its own)

        static Applied synchronous(int every, int64_t step, bool own_loop, bool ghosts) {
            Applied a = at(every, step);
            a.check_in = own_loop && !ghosts; a.ghosts = ghosts;
            return a;
        }
        static Applied asynchronous(int every, int64_t measured_at, int64_t step) {
            Applied a = at(every, measured_at);
            a.headroom_steps = (double)(step - measured_at); a.check_in = true;
            return a;
        }
        static Applied collective(int every, int64_t step, int late, bool check_in, bool ghosts) {
            Applied a = at(every, step);
            a.horizon = every + std::max(late - 1, 0); a.headroom_steps = (double)(1 + late);
            a.min_check_in = std::max(MIN_CHECK_IN, late + 2); a.check_in = check_in;
            a.keeps_step = false; a.ghosts = ghosts;
            return a;
        }
        static Applied lazy_single(int every, int64_t step, bool own_loop) {
            Applied a = at(every, step);
            a.check_in = own_loop; a.single = true;
            return a;
        }
      private:
        static Applied at(int every, int64_t step) { Applied a; a.every = a.horizon = every; a.measured_at = step; return a; }
    };
    enum Action { KEEP, LOOK_AGAIN, PRUNE, SEARCH };
    struct Decision {
        Action action; int k;           // LOOK_AGAIN: in k steps from the measured one
        double ahead; bool grown;       // the drift allowed for | the inner skin grew (PRUNE or SEARCH follows: the radius changed)
    };

    // largest k < every such that a displacement of d now stays within CHECK_IN_SLACK·margin for k more steps (0: none worth a check of its own)
    int steps_within(double d, double margin, int64_t steps_so_far, const Applied& a) const {
        const double per_step = drift_ahead(d, steps_so_far, 1);
        if (!(per_step > 0)) return 0;
        const double fit = std::floor((CHECK_IN_SLACK * margin - d) / per_step);
        if (!(fit >= a.min_check_in)) return 0;
        const int k = (int)std::min<double>(fit, a.every - 1);
        return k >= a.min_check_in ? k : 0;
    }

    // A list that cannot be vouched for over a whole interval (the fastest atom could use up the remaining slack in `every` steps)
    // may still be good for k < every steps: instead of giving it up now, look again in k steps.  Light, fast atoms (hydrogens at
    // 0.5 fs: 0.06 nm of possible drift per 10 steps against 0.1 nm of slack) otherwise cost a search at nearly every interval.
    // A prune is only as good as the outer list behind it: if that is used up (with the headroom of the steps until the prune
    // runs), search again instead of running a prune pass that would have to be thrown away.
    // d_outer(): the displacement since the outer search, asked for only when a prune is about to be decided (the synchronous
    // form measures it then).
    template <class OuterDisp> Decision decide(const Measured& m, const Applied& a, OuterDisp&& d_outer) {
        Decision r{SEARCH, 0, 0.0, false};
        if (!std::isinf(m.d)) {
            const double ahead = r.ahead = drift_ahead(m.d, m.steps, a.horizon);
            if (!a.single) r.grown = grow_inner_skin(ahead, a.ghosts);
            const double margin = a.single ? skin : skin_in;
            if (a.keeps_step) next_check_step = -1;
            if (!r.grown && covered(m.d, ahead, margin)) { r.action = KEEP; return r; }
            if (!r.grown && a.check_in) {
                if ((r.k = steps_within(m.d, margin, m.steps, a)) != 0) {
                    if (a.keeps_step) next_check_step = a.measured_at + r.k;
                    r.action = LOOK_AGAIN;
                    return r;
                }
            }
        }
        if (a.single) return r;
        const double d_out = d_outer();      // (first: where this measures, it brings the speed the headroom goes by)
        const double headroom = last_vmax * cur_dt * HEADROOM_STRETCH * a.headroom_steps;
        if (covered(d_out, headroom, prune_margin())) r.action = PRUNE;
        return r;
    }
    Decision decide(const Measured& m, const Applied& a) { return decide(m, a, [&] { return m.d_outer; }); }
};

}   // namespace mhip
