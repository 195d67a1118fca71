// Stand-alone check of molly.jl_amd/csrc/list_policy.h (tests/test_list_policy_host.py compiles and runs it): known answers of the
// decision in its call forms, then a deterministic sweep that asserts the safety property the rule exists for.  Exit status 0 = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "list_policy.h"

using mhip::ListPolicy;
using Applied = ListPolicy::Applied;
using Measured = ListPolicy::Measured;
using Decision = ListPolicy::Decision;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(1.0, std::fmax(std::fabs(a), std::fabs(b))); }
static const char* const NAMES[4] = {"keep", "look again", "prune", "search"};

// the state of the known-answer table: dt 0.002, skin 0.2, skin_in 0.1, outer_margin 0.1 (prune_margin 0.2), pruned at step 0
static ListPolicy table_state(double v_max, double v_before) {
    ListPolicy p;
    p.inner_skin_fixed = false;
    p.skin = 0.2; p.skin_in = 0.1; p.rc_max = 1.0; p.outer_margin = 0.1; p.cur_dt = 0.002;
    p.last_vmax = v_before;
    p.measured(v_max);
    return p;
}

static void known_answers() {
    const int every = 10;
    {   // first measurement of a run (no speed before): growth 1.25
        ListPolicy p = table_state(1.0, 0.0);
        const Decision r = p.decide(Measured{0.010, 0.020, 10}, Applied::synchronous(every, 10, true, false));
        CHECK(r.action == ListPolicy::KEEP && near(r.ahead, 0.025) && !r.grown && p.skin_in == 0.1 && p.next_check_step == -1, "%s ahead %.17g skin_in %.17g", NAMES[r.action], r.ahead, p.skin_in);
        CHECK(near(p.prune_margin(), 0.2) && p.n_disp_checks == 1 && p.prev_vmax == 0.0 && p.last_vmax == 1.0, "prune_margin %.17g", p.prune_margin());
    }
    {   // not good for a whole interval, but for 8 steps
        ListPolicy p = table_state(1.0, 1.0);
        const Decision r = p.decide(Measured{0.030, 0.040, 20}, Applied::synchronous(every, 20, true, false));
        CHECK(r.action == ListPolicy::LOOK_AGAIN && r.k == 8 && near(r.ahead, 0.022) && p.next_check_step == 28, "%s k %d ahead %.17g next %lld", NAMES[r.action], r.k, r.ahead, (long long)p.next_check_step);
        CHECK(p.check_due(28, every) && p.check_due(30, every) && !p.check_due(27, every), "check_due");
        // … the same outside a run that owns its loop: nobody would come back in 8 steps, so the list is pruned
        ListPolicy q = table_state(1.0, 1.0);
        const Decision s = q.decide(Measured{0.030, 0.040, 20}, Applied::synchronous(every, 20, false, false));
        CHECK(s.action == ListPolicy::PRUNE && q.next_check_step == -1, "%s", NAMES[s.action]);
    }
    {   // no k >= 3 fits: prune, the outer list is good for it
        ListPolicy p = table_state(1.0, 1.0);
        const Decision r = p.decide(Measured{0.045, 0.040, 20}, Applied::synchronous(every, 20, true, false));
        CHECK(r.action == ListPolicy::PRUNE && p.next_check_step == -1, "%s", NAMES[r.action]);
    }
    {   // … the outer list is used up: search
        ListPolicy p = table_state(1.0, 1.0);
        const Decision r = p.decide(Measured{0.045, 0.150, 20}, Applied::synchronous(every, 20, true, false));
        CHECK(r.action == ListPolicy::SEARCH, "%s", NAMES[r.action]);
    }
    {   // the top speed doubled: the inner skin grows to all of skin, which leaves the outer list prune_margin 0.1
        ListPolicy p = table_state(2.0, 1.0);
        const Decision r = p.decide(Measured{0.020, 0.040, 10}, Applied::synchronous(every, 10, true, false));
        CHECK(r.action == ListPolicy::PRUNE && r.grown && near(r.ahead, 0.08) && p.skin_in == 0.2 && p.skin_in_adapted == 0.2 && near(p.prune_margin(), 0.1), "%s ahead %.17g skin_in %.17g", NAMES[r.action], r.ahead, p.skin_in);
        CHECK(p.want_margin_zero, "outer margin 0.1 <= 2 * 0.2 - 0.2 + 0.02 has no second prune to serve");
        ListPolicy q = table_state(2.0, 1.0);
        const Decision s = q.decide(Measured{0.020, 0.050, 10}, Applied::synchronous(every, 10, true, false));
        CHECK(s.action == ListPolicy::SEARCH && s.grown && q.skin_in == 0.2, "%s skin_in %.17g", NAMES[s.action], q.skin_in);
    }
    {   // driven from outside (no time step): the empirical drift 1.5 * d * every / steps
        ListPolicy p = table_state(7.0, 3.0);
        p.cur_dt = 0; p.skin_in = 0.2; p.outer_margin = 0;
        const Decision r = p.decide(Measured{0.030, 0.040, 20}, Applied::synchronous(every, 20, false, false));
        CHECK(r.action == ListPolicy::KEEP && near(r.ahead, 0.0225), "%s ahead %.17g", NAMES[r.action], r.ahead);
    }
    {   // collective form, applied one step late: the caller is handed k, next_check_step is not the policy's to set
        ListPolicy p = table_state(1.0, 1.0);
        p.next_check_step = 77;
        const Decision r = p.decide(Measured{0.038, 0.040, 20}, Applied::collective(every, 20, 1, true, true));
        CHECK(r.action == ListPolicy::LOOK_AGAIN && r.k == 5 && p.next_check_step == 77, "%s k %d", NAMES[r.action], r.k);
        // … three steps late, k = 5 > late + 1 = 4 still stands, but the drift horizon is every + 2; four steps late it does not
        ListPolicy q = table_state(1.0, 1.0);
        CHECK(q.decide(Measured{0.038, 0.040, 20}, Applied::collective(every, 20, 3, true, true)).action == ListPolicy::LOOK_AGAIN, "late 3");
        CHECK(q.decide(Measured{0.038, 0.040, 20}, Applied::collective(every, 20, 4, true, true)).action == ListPolicy::PRUNE, "late 4");
        CHECK(q.decide(Measured{0.038, 0.040, 20}, Applied::collective(every, 20, 1, false, true)).action == ListPolicy::PRUNE, "no check_in pointer");
    }
    {   // asynchronous form: the outer test leaves headroom for the steps between measurement and prune (1.25 * v_max * dt each)
        ListPolicy p = table_state(1.0, 1.0);      // prune_margin 0.2: 2 * (0.0965 + 0.0025) > 0.196 >= 2 * 0.0965
        CHECK(p.decide(Measured{0.045, 0.0965, 20}, Applied::synchronous(every, 20, true, false)).action == ListPolicy::PRUNE, "no headroom");
        CHECK(p.decide(Measured{0.045, 0.0965, 20}, Applied::asynchronous(every, 20, 21)).action == ListPolicy::SEARCH, "one step of headroom");
    }
    {   // the lazy single list: the same test against skin, no outer list to prune from
        ListPolicy p = table_state(1.0, 1.0);
        p.outer_margin = 0;
        CHECK(p.decide(Measured{0.070, 0.0, 20}, Applied::lazy_single(every, 20, true)).action == ListPolicy::KEEP && p.skin_in == 0.1, "lazy keep");
        const Decision r = p.decide(Measured{0.080, 0.0, 20}, Applied::lazy_single(every, 20, true));      // (0.098 - 0.080) / 0.0022 = 8.18
        CHECK(r.action == ListPolicy::LOOK_AGAIN && r.k == 8 && p.next_check_step == 28, "%s k %d", NAMES[r.action], r.k);
        CHECK(p.decide(Measured{0.095, 0.0, 20}, Applied::lazy_single(every, 20, true)).action == ListPolicy::SEARCH && p.next_check_step == -1, "lazy search");
    }
    {   // no inner list to vouch for (+inf): only the outer test is made; a NaN measurement never keeps a list
        ListPolicy p = table_state(1.0, 1.0);
        CHECK(p.decide(Measured{INFINITY, 0.040, 20}, Applied::synchronous(every, 20, true, false)).action == ListPolicy::PRUNE && p.skin_in == 0.1, "inf, outer good");
        CHECK(p.decide(Measured{INFINITY, 0.150, 20}, Applied::synchronous(every, 20, true, false)).action == ListPolicy::SEARCH, "inf, outer used up");
        CHECK(p.decide(Measured{NAN, 0.040, 20}, Applied::synchronous(every, 20, true, false)).action == ListPolicy::PRUNE, "NaN d");
        CHECK(p.decide(Measured{0.010, NAN, 20}, Applied::synchronous(every, 20, true, false)).action == ListPolicy::KEEP, "NaN d_outer is not looked at while the inner list stands");
        CHECK(p.decide(Measured{0.045, NAN, 20}, Applied::synchronous(every, 20, true, false)).action == ListPolicy::SEARCH, "NaN d_outer");
        CHECK(!ListPolicy::covered(NAN, 0, 1) && !ListPolicy::covered(0, NAN, 1) && !ListPolicy::covered(0, 0, NAN) && ListPolicy::covered(0.49, 0, 1) && !ListPolicy::covered(0.4901, 0, 1), "covered");
    }
    {   // a fixed inner skin (MOLLYHIP_INNER_SKIN_FIXED) never grows; one that is all of skin cannot
        ListPolicy p = table_state(2.0, 1.0);
        p.inner_skin_fixed = true;
        const Decision r = p.decide(Measured{0.020, 0.040, 10}, Applied::synchronous(every, 10, true, false));
        CHECK(!r.grown && p.skin_in == 0.1 && r.action == ListPolicy::LOOK_AGAIN && r.k == 3 && !p.want_margin_zero, "%s k %d", NAMES[r.action], r.k);      // (0.049 - 0.020) / 0.008 = 3.6
    }
    {   // an outer list outrun within two intervals of its search, three times in a row: the dual list is given up
        ListPolicy p;
        p.last_outer_step = 100;
        CHECK(!p.outer_outrun(110, every) && !p.outer_outrun(120, every), "two");
        CHECK(!p.outer_outrun(121, every) && p.early_outer == 0, "a late one starts the count again");
        CHECK(!p.outer_outrun(105, every) && !p.outer_outrun(105, every) && p.outer_outrun(105, every), "three in a row");
    }
    {   // the inner skin at the start: floor (or what a run grew it to) | all of skin
        ListPolicy p;
        p.skin = 0.2; p.skin_in_adapted = 0.15;
        p.start_inner_skin(true, 0.1); CHECK(p.skin_in == 0.15, "grown stays");
        p.start_inner_skin(true, 0.1, false); CHECK(p.skin_in == 0.1, "floor");
        p.start_inner_skin(true, 0.25); CHECK(p.skin_in == 0.2, "never more than skin");
        p.start_inner_skin(false, 0.1); CHECK(p.skin_in == 0.2, "all of skin");
    }
}

// fixed-seed LCG (Knuth's MMIX multiplier), the top 53 bits as a double in [0, 1): the same sequence everywhere
static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uni() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg_state >> 11) * (1.0 / 9007199254740992.0); }
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }
static int pick(int n) { return (int)(uni() * n); }

static void sweep(long n_inputs) {
    long count[4] = {0, 0, 0, 0};
    for (long i = 0; i < n_inputs && failures < 20; ++i) {
        const int form = (int)(i % 4);      // 0 synchronous, 1 asynchronous, 2 collective, 3 lazy single
        static const int EVERY[3] = {5, 10, 20};
        const int every = EVERY[pick(3)];
        ListPolicy p;
        p.inner_skin_fixed = pick(8) == 0;
        p.skin = uni(0.1, 0.3);
        p.skin_in = form == 3 || pick(4) == 0 ? p.skin : p.skin * uni(0.3, 1.0);
        p.rc_max = 1.0;
        p.outer_margin = form == 3 || pick(4) == 0 ? 0.0 : uni(0.0, 0.2);
        p.cur_dt = pick(4) == 0 ? 0.0 : uni(0.0005, 0.002);
        const double v = uni(0.2, 3.0), v_before = pick(5) == 0 ? 0.0 : v * uni(0.7, 1.3);
        p.last_vmax = v_before;
        p.measured(v);
        const double margin0 = form == 3 ? p.skin : p.skin_in, skin_in0 = p.skin_in;
        const Measured m{pick(16) == 0 ? (double)INFINITY : uni(0.0, 0.6) * margin0, uni(0.0, 0.75) * p.prune_margin() + uni(0.0, 0.02), 1 + pick(2 * every)};
        const int late = pick(3), late_async = 1 + pick(2);
        const bool own_loop = pick(4) != 0, ghosts = form == 2 && pick(2) == 0;
        const int64_t step = 1000;
        const Applied a = form == 0 ? Applied::synchronous(every, step, own_loop, ghosts) : form == 1 ? Applied::asynchronous(every, step, step + late_async)
                        : form == 2 ? Applied::collective(every, step, late, own_loop, ghosts) : Applied::lazy_single(every, step, own_loop);
        p.next_check_step = 7;
        const Decision r = p.decide(m, a);
        ++count[r.action];

        // the form's row of the table, restated
        const int horizon = form == 2 ? every + (late > 1 ? late - 1 : 0) : every;
        const double headroom_steps = form == 1 ? late_async : form == 2 ? 1 + late : 0;
        const bool check_in_ok = form == 1 || own_loop;
        const int k_min = form == 2 && late + 2 > 3 ? late + 2 : 3;
        const double growth = v_before > 0 ? std::fmin(std::fmax(v / v_before, 1.1), 3.0) : 1.25;
        const double per_step = p.cur_dt > 0 ? v * growth * p.cur_dt : 1.5 * m.d / (double)m.steps;
        const double margin = form == 3 ? p.skin : p.skin_in;      // (after the decision: a grown skin is the one that counts)
        const bool listed = !std::isinf(m.d);
        const bool outer_ok = ListPolicy::covered(m.d_outer, v * p.cur_dt * 1.25 * headroom_steps, p.prune_margin());
#define CASE "input %ld form %d every %d dt %.6f d %.6f d_outer %.6f steps %lld skin %.4f skin_in %.4f -> %.4f margin %.4f v %.3f (before %.3f) late %d/%d own %d: %s k %d ahead %.6f", \
             i, form, every, p.cur_dt, m.d, m.d_outer, (long long)m.steps, p.skin, skin_in0, p.skin_in, p.outer_margin, v, v_before, late, late_async, (int)own_loop, NAMES[r.action], r.k, r.ahead
        CHECK(p.skin_in >= skin_in0 && p.skin_in <= p.skin && r.grown == (p.skin_in > skin_in0), CASE);
        CHECK(!r.grown || (form != 3 && !p.inner_skin_fixed && listed && near(p.skin_in, std::fmin(p.skin, 3.0 * r.ahead / 0.98))), CASE);
        if (listed) CHECK(near(r.ahead, per_step * horizon), CASE);
        switch (r.action) {
        case ListPolicy::KEEP:
            CHECK(listed && !r.grown && ListPolicy::covered(m.d, per_step * horizon, margin), CASE);
            break;
        case ListPolicy::LOOK_AGAIN:
            CHECK(listed && !r.grown && check_in_ok && r.k >= 3 && r.k >= k_min && r.k <= every - 1 && m.d + r.k * per_step <= 0.49 * margin, CASE);
            CHECK(!ListPolicy::covered(m.d, per_step * horizon, margin), CASE);      // (a whole interval was not vouched for)
            break;
        case ListPolicy::PRUNE:
            CHECK(form != 3 && outer_ok, CASE);
            break;
        default:
            CHECK(form == 3 || !outer_ok, CASE);
            break;
        }
        if (r.action == ListPolicy::PRUNE || r.action == ListPolicy::SEARCH) {      // the list was not given up while the rule could vouch for it
            const bool k_fits = check_in_ok && per_step > 0 && std::fmin(std::floor((0.49 * margin - m.d) / per_step), every - 1) >= k_min;
            CHECK(!listed || r.grown || (!ListPolicy::covered(m.d, per_step * horizon, margin) && !k_fits), CASE);
        }
        // who keeps the look-again step: the engine's own loops in next_check_step (cleared by every decision on a list), the collective caller itself
        const int64_t next = form == 2 || !listed ? 7 : r.action == ListPolicy::LOOK_AGAIN ? step + r.k : -1;
        CHECK(p.next_check_step == next, CASE);
        if (r.grown) CHECK(p.want_margin_zero == (!ghosts && p.outer_margin > 0 && p.outer_margin <= 2.0 * p.skin_in - p.skin + 0.02), CASE);
        else CHECK(!p.want_margin_zero, CASE);
#undef CASE
    }
    std::printf("sweep: %ld inputs:", n_inputs);
    for (int k = 0; k < 4; ++k) {
        std::printf(" %s %ld (%.1f %%)", NAMES[k], count[k], 100.0 * (double)count[k] / (double)n_inputs);
        CHECK(count[k] * 50 >= n_inputs, "under 2 %% of the inputs ended in '%s'", NAMES[k]);
    }
    std::printf("\n");
}

int main() {
    known_answers();
    sweep(200000);
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("list policy: all checks passed\n");
    return failures ? 1 : 0;
}
