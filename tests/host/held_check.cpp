// Stand-alone check of molly.jl_amd/csrc/held.h (tests/test_held_host.py compiles and runs it): known answers — for every event the
// full flag vector before and after, from at least two starting states, written down by hand from the header's table — then a sweep
// over every flag combination × every event for the properties the engine relies on (the header lists them).  Exit status 0 = pass.
#include <cstdio>

#include "held.h"

using namespace mhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the columns of the table, as bits() orders them
enum : unsigned {
    S = 1u << 0,    // stale
    M = 1u << 1,    // coords_moved
    X = 1u << 2,    // export_needs_search
    I = 1u << 3,    // inner_valid
    O = 1u << 4,    // prune_disp_exceeded
    F = 1u << 5,    // frc_valid
    T = 1u << 6,    // frc_run_total
    P = 1u << 7,    // frc_before_set_state
    C = 1u << 8,    // state_set
    A = 1u << 9,    // params_set
    W = 1u << 10,   // state_pending
    V = 1u << 11,   // vel_check_due
    K = 1u << 12,   // trk_issued
    L = 1u << 13,   // prune_pending
    N = 1u << 14,   // interior_done
    ALL = (1u << Held::N_FLAGS) - 1
};
static const unsigned RUN = I | F | T | C | A;      // the end of a run over a dual list: lists, total forces, nothing pending

struct Event { const char* name; void (*apply)(Held&); unsigned may_change; };
static const Event events[] = {
    {"atoms_replaced(false)", [](Held& h) { h.atoms_replaced(false); }, S | F | K},
    {"atoms_replaced(true)", [](Held& h) { h.atoms_replaced(true); }, S | M | F | T | W | K | N},
    {"interactions_changing()", [](Held& h) { h.interactions_changing(); }, T | P},
    {"params_changed(false)", [](Held& h) { h.params_changed(false); }, F | A},
    {"params_changed(true)", [](Held& h) { h.params_changed(true); }, S | F | A},
    {"exceptions_changed()", [](Held& h) { h.exceptions_changed(); }, S},
    {"terms_changed()", [](Held& h) { h.terms_changed(); }, T},
    {"pme_changed()", [](Held& h) { h.pme_changed(); }, F},
    {"lists_voided()", [](Held& h) { h.lists_voided(); }, S},
    {"box_changed(false)", [](Held& h) { h.box_changed(false); }, S | F | C},
    {"box_changed(true)", [](Held& h) { h.box_changed(true); }, S | F | T | P | C},
    {"state_write_begins()", [](Held& h) { (void)h.state_write_begins(); }, P | W},
    {"coords_written(true)", [](Held& h) { h.coords_written(true); }, S | M | F | C},
    {"coords_written(false)", [](Held& h) { h.coords_written(false); }, S | M | F | C},
    {"state_compared(false, false)", [](Held& h) { h.state_compared(false, false); }, M | F | P | W | K},
    {"state_compared(false, true)", [](Held& h) { h.state_compared(false, true); }, M | F | P | W | K},
    {"state_compared(true, false)", [](Held& h) { h.state_compared(true, false); }, M | F | P | W | K},
    {"state_compared(true, true)", [](Held& h) { h.state_compared(true, true); }, M | F | P | W | K},
    {"moved_coords_taken(false, false)", [](Held& h) { (void)h.moved_coords_taken(false, false); }, M | V},
    {"moved_coords_taken(false, true)", [](Held& h) { (void)h.moved_coords_taken(false, true); }, M | V},
    {"moved_coords_taken(true, false)", [](Held& h) { (void)h.moved_coords_taken(true, false); }, M | V},
    {"moved_coords_taken(true, true)", [](Held& h) { (void)h.moved_coords_taken(true, true); }, M | V},
    {"export_wants_search()", [](Held& h) { h.export_wants_search(); }, X},
    {"vel_check_taken()", [](Held& h) { h.vel_check_taken(); }, V},
    {"lists_searched(true)", [](Held& h) { h.lists_searched(true); }, S | M | X | I | O | T},
    {"lists_searched(false)", [](Held& h) { h.lists_searched(false); }, S | M | X | T},
    {"inner_list_made(READ_NOW, false)", [](Held& h) { h.inner_list_made(Held::Prune::READ_NOW, false); }, I | O | L},
    {"inner_list_made(READ_NOW, true)", [](Held& h) { h.inner_list_made(Held::Prune::READ_NOW, true); }, I | O | L},
    {"inner_list_made(READ_LATE)", [](Held& h) { h.inner_list_made(Held::Prune::READ_LATE); }, I | O | L},
    {"inner_list_made(ADOPTED)", [](Held& h) { h.inner_list_made(Held::Prune::ADOPTED); }, I | O},
    {"prune_wanted()", [](Held& h) { h.prune_wanted(); }, I},
    {"outrun_taken()", [](Held& h) { h.outrun_taken(); }, O},
    {"prune_read()", [](Held& h) { h.prune_read(); }, L},
    {"forces_total()", [](Held& h) { h.forces_total(); }, F},
    {"forces_partial()", [](Held& h) { h.forces_partial(); }, F},
    {"drifted()", [](Held& h) { h.drifted(); }, F},
    {"run_begins()", [](Held& h) { h.run_begins(); }, T},
    {"run_ended(true)", [](Held& h) { h.run_ended(true); }, T},
    {"run_ended(false)", [](Held& h) { h.run_ended(false); }, T},
    {"check_issued()", [](Held& h) { h.check_issued(); }, K},
    {"check_read()", [](Held& h) { h.check_read(); }, K},
    {"interior_pass(true)", [](Held& h) { h.interior_pass(true); }, N},
    {"interior_pass(false)", [](Held& h) { h.interior_pass(false); }, N},
};
static const int n_events = (int)(sizeof(events) / sizeof(events[0]));

static const Event& event(const char* name) {
    for (const Event& e : events) { const char *a = e.name, *b = name; while (*a && *a == *b) { ++a; ++b; } if (!*a && !*b) return e; }
    ++failures; std::printf("FAIL: no event %s\n", name);
    return events[0];
}
static unsigned after(const char* name, unsigned before) { Held h = Held::from_bits(before); event(name).apply(h); return h.bits(); }
static int n_known = 0;
static void known(const char* name, unsigned before, unsigned expect) {
    const unsigned got = after(name, before);
    ++n_known;
    CHECK(got == expect, "%s from %04x: %04x, expected %04x", name, before, got, expect);
}
// an event that sets and clears unconditionally: from nothing, from everything, from the end of a run
static void known_uncond(const char* name, unsigned set, unsigned clear) {
    const unsigned starts[3] = {0u, ALL, RUN};
    for (unsigned s : starts) known(name, s, (s | set) & ~clear);
}

static void known_answers() {
    CHECK(Held().bits() == S, "a new context: %04x", Held().bits());      // stale, nothing else
    CHECK(Held::from_bits(RUN).bits() == RUN && Held::from_bits(ALL).bits() == ALL && Held::from_bits(0).bits() == 0, "bits round trip");
    for (int k = 0; k < Held::N_FLAGS; ++k) CHECK(Held::from_bits(1u << k).bits() == 1u << k, "bit %d round trip", k);
    {   // the accessors read the columns they are named for
        const Held h = Held::from_bits(ALL), z = Held::from_bits(0);
        CHECK(h.stale() && h.coords_moved() && h.export_needs_search() && h.inner_valid() && h.prune_disp_exceeded() && h.frc_valid() && h.frc_run_total() && h.frc_before_set_state(), "accessors, all set");
        CHECK(h.state_set() && h.params_set() && h.state_pending() && h.vel_check_due() && h.trk_issued() && h.prune_pending() && h.interior_done(), "accessors, all set");
        CHECK(!z.stale() && !z.coords_moved() && !z.export_needs_search() && !z.inner_valid() && !z.prune_disp_exceeded() && !z.frc_valid() && !z.frc_run_total() && !z.frc_before_set_state(), "accessors, none set");
        CHECK(!z.state_set() && !z.params_set() && !z.state_pending() && !z.vel_check_due() && !z.trk_issued() && !z.prune_pending() && !z.interior_done(), "accessors, none set");
        CHECK(Held::from_bits(S).stale() && Held::from_bits(M).coords_moved() && Held::from_bits(X).export_needs_search() && Held::from_bits(I).inner_valid() && Held::from_bits(O).prune_disp_exceeded(), "single accessors");
        CHECK(Held::from_bits(F).frc_valid() && Held::from_bits(T).frc_run_total() && Held::from_bits(P).frc_before_set_state() && Held::from_bits(C).state_set() && Held::from_bits(A).params_set(), "single accessors");
        CHECK(Held::from_bits(W).state_pending() && Held::from_bits(V).vel_check_due() && Held::from_bits(K).trk_issued() && Held::from_bits(L).prune_pending() && Held::from_bits(N).interior_done(), "single accessors");
    }
    // ---- the setters
    known_uncond("atoms_replaced(false)", S, F | K);
    known_uncond("atoms_replaced(true)", S, M | F | T | W | K | N);
    known_uncond("interactions_changing()", 0, T | P);
    known_uncond("params_changed(false)", A, F);
    known_uncond("params_changed(true)", S | A, F);
    known_uncond("exceptions_changed()", S, 0);
    known_uncond("terms_changed()", 0, T);
    known_uncond("pme_changed()", 0, F);
    known_uncond("lists_voided()", S, 0);
    known_uncond("box_changed(false)", S, F | C);
    known_uncond("box_changed(true)", S, F | T | P | C);
    // ---- a state written, compared, taken
    known("state_write_begins()", 0, W);                          // first write, no forces: nothing to remember
    known("state_write_begins()", F, F | P | W);                  // first write over current forces: remembered
    known("state_write_begins()", P, W);                          // … a stale memory is overwritten by "no forces"
    known("state_write_begins()", RUN, RUN | P | W);
    known("state_write_begins()", W | F, W | F);                  // a second write before the read-back: the first one decided
    known("state_write_begins()", ALL, ALL);
    { Held h = Held::from_bits(F); CHECK(h.state_write_begins(), "the first write zeroes the words"); CHECK(!h.state_write_begins(), "the second does not"); }
    known("coords_written(true)", 0, M | C);                      // lists with a skin live on, to be measured
    known("coords_written(true)", RUN, (RUN | M) & ~F);
    known("coords_written(true)", S | F, S | C);                  // no lists: nothing to measure
    known("coords_written(true)", ALL, ALL & ~F);
    known("coords_written(false)", 0, S | C);                     // lists without a skin: void at once
    known("coords_written(false)", RUN, (RUN | S) & ~F);
    known("coords_written(false)", ALL, ALL & ~F);
    known("state_compared(false, false)", RUN | P | W | M | K, RUN | K);      // the same state handed back: everything stands (frc was already on here)
    known("state_compared(false, false)", P | W | M | I, F | I);              // … and the forces are current again
    known("state_compared(false, false)", P | W | M | S, S);                  // … but not without lists
    known("state_compared(false, false)", W | M, 0);                          // … nor if they were not current before
    known("state_compared(false, false)", ALL, ALL & ~(W | M | P));
    known("state_compared(false, true)", P | W | M | K, F);                   // new velocities: the check in flight is dropped
    known("state_compared(false, true)", ALL, ALL & ~(W | M | P | K));
    known("state_compared(true, false)", P | W | M | K | I, M | I);           // new coordinates: moved stays, no forces, no check
    known("state_compared(true, false)", ALL, ALL & ~(W | P | K));
    known("state_compared(true, true)", P | W | M | K, M);
    known("state_compared(true, true)", 0, 0);
    known("moved_coords_taken(true, true)", 0, V);                // new velocities on lists that live on
    known("moved_coords_taken(true, true)", M, V);                // … with moved coordinates: both, measure now
    known("moved_coords_taken(true, true)", M | S, S);            // … without lists: the search will see to it
    known("moved_coords_taken(true, true)", ALL, ALL & ~M);
    known("moved_coords_taken(true, false)", 0, 0);               // lists without a skin are never kept across new velocities
    known("moved_coords_taken(true, false)", M, V);
    known("moved_coords_taken(false, true)", M | I, I);
    known("moved_coords_taken(false, true)", RUN, RUN);
    known("moved_coords_taken(false, false)", M | V, V);
    known("moved_coords_taken(false, false)", 0, 0);
    {   // the answer: measure now?
        Held a = Held::from_bits(M), b = Held::from_bits(M | S), c = Held::from_bits(0);
        CHECK(a.moved_coords_taken(false, true), "moved, lists alive: measure"); CHECK(!b.moved_coords_taken(false, true), "moved, stale: no"); CHECK(!c.moved_coords_taken(true, true), "not moved: no");
    }
    known_uncond("export_wants_search()", X, 0);
    known_uncond("vel_check_taken()", 0, V);
    // ---- the lists
    known_uncond("lists_searched(true)", 0, S | M | X | I | O | T);
    known_uncond("lists_searched(false)", 0, S | M | X | T);
    known_uncond("inner_list_made(READ_NOW, false)", I, O | L);
    known_uncond("inner_list_made(READ_NOW, true)", I | O, L);
    known_uncond("inner_list_made(READ_LATE)", I | L, O);
    known_uncond("inner_list_made(ADOPTED)", I, O);
    known_uncond("prune_wanted()", 0, I);
    known_uncond("outrun_taken()", 0, O);
    known_uncond("prune_read()", 0, L);
    // ---- the forces and the runs
    known_uncond("forces_total()", F, 0);
    known_uncond("forces_partial()", 0, F);
    known_uncond("drifted()", 0, F);
    known_uncond("run_begins()", 0, T);
    known_uncond("run_ended(true)", T, 0);
    known_uncond("run_ended(false)", 0, T);
    known_uncond("check_issued()", K, 0);
    known_uncond("check_read()", 0, K);
    known_uncond("interior_pass(true)", N, 0);
    known_uncond("interior_pass(false)", 0, N);
    // ---- the queries
    CHECK(Held::from_bits(RUN).reusable_run_forces(), "the end of a run");
    CHECK(!Held::from_bits(RUN & ~T).reusable_run_forces() && !Held::from_bits(RUN & ~F).reusable_run_forces() && !Held::from_bits(RUN | S).reusable_run_forces() && !Held::from_bits(RUN | M).reusable_run_forces(), "each of the four alone loses the run's forces");
    CHECK(Held::from_bits(F | T).reusable_run_forces(), "a single list has no inner list to ask for");
    CHECK(Held::from_bits(I).inner_list_stands() && !Held::from_bits(I | S).inner_list_stands() && !Held::from_bits(0).inner_list_stands() && Held::from_bits(ALL & ~S).inner_list_stands(), "inner_list_stands");
    CHECK(Held::from_bits(I).split_pass_ok(true, false) && !Held::from_bits(0).split_pass_ok(true, false), "split pass over a dual list: the inner list decides");
    CHECK(Held::from_bits(0).split_pass_ok(false, false) && !Held::from_bits(I).split_pass_ok(false, true), "split pass over a single list: not a lazily kept one");
    // ---- a life: create, set, run, hand the same state back, run on; then move an atom
    {
        Held h;
        h.interactions_changing(); h.params_changed(false); h.state_write_begins(); h.coords_written(true);
        CHECK(h.bits() == (S | A | C | W), "set up: %04x", h.bits());
        h.state_compared(true, true); (void)h.moved_coords_taken(true, true); h.run_begins(); h.vel_check_taken(); h.lists_searched(true);
        CHECK(h.bits() == (A | C), "searched: %04x", h.bits());
        h.inner_list_made(Held::Prune::READ_NOW, false); h.forces_total(); h.drifted(); h.forces_total(); h.run_ended(true);
        CHECK(h.bits() == RUN && h.reusable_run_forces(), "run ended: %04x", h.bits());
        h.state_write_begins(); h.coords_written(true);
        CHECK(h.bits() == ((RUN | P | W | M) & ~F) && !h.reusable_run_forces(), "state handed back: %04x", h.bits());
        h.state_compared(false, false);
        CHECK(h.bits() == RUN && !h.moved_coords_taken(false, true) && h.reusable_run_forces(), "… unchanged: %04x", h.bits());
        h.state_write_begins(); h.coords_written(true); h.state_compared(true, false);
        CHECK(h.bits() == ((RUN | M) & ~F) && !h.reusable_run_forces() && h.moved_coords_taken(false, true) && h.bits() == (RUN & ~F), "… an atom moved: %04x", h.bits());
    }
}

static bool is(const Event& e, const char* prefix) { const char* a = e.name; while (*prefix && *a == *prefix) { ++a; ++prefix; } return !*prefix; }

static void sweep() {
    long long n = 0;
    for (unsigned b = 0; b <= ALL; ++b) {
        const Held before = Held::from_bits(b);
        // 5. (a property of the states)
        if (before.reusable_run_forces()) CHECK(before.frc_valid() && before.frc_run_total() && !before.stale() && !before.coords_moved(), "state %04x", b);
        CHECK(before.inner_list_stands() == (before.inner_valid() && !before.stale()), "state %04x", b);
        for (int k = 0; k < n_events; ++k) {
            const Event& e = events[k];
            Held h = before; e.apply(h);
            const unsigned a = h.bits(), on = a & ~b, off = b & ~a;
            ++n;
            // the frame: an event touches only the columns its row of the table names
            CHECK(((a ^ b) & ~e.may_change) == 0, "%s from %04x: changed %04x", e.name, b, a ^ b);
            // 1.
            if (is(e, "lists_searched")) CHECK(!(a & (S | M | X | T)), "%s from %04x: %04x", e.name, b, a);
            // 2. who may turn what on, who may clear stale
            if (on & F) CHECK(is(e, "forces_total") || (is(e, "state_compared(false") && (b & P) && !(b & S)), "%s from %04x turned frc on", e.name, b);
            if (on & T) CHECK(is(e, "run_ended(true)"), "%s from %04x turned frc_run_total on", e.name, b);
            if (off & S) CHECK(is(e, "lists_searched"), "%s from %04x cleared stale", e.name, b);
            if (on & I) CHECK(is(e, "inner_list_made"), "%s from %04x set inner_valid", e.name, b);
            if (on & K) CHECK(is(e, "check_issued"), "%s from %04x set trk_issued", e.name, b);
            if (on & L) CHECK(is(e, "inner_list_made(READ_LATE)"), "%s from %04x set prune_pending", e.name, b);
            if (on & N) CHECK(is(e, "interior_pass(true)"), "%s from %04x set interior_done", e.name, b);
            if (on & O) CHECK(is(e, "inner_list_made(READ_NOW, true)"), "%s from %04x set prune_disp_exceeded", e.name, b);
            // 3. the voiding calls
            if (is(e, "atoms_replaced") || is(e, "exceptions_changed") || is(e, "lists_voided") || is(e, "box_changed") || is(e, "params_changed(true)"))
                CHECK(h.stale() && !h.reusable_run_forces() && !h.inner_list_stands(), "%s from %04x: %04x", e.name, b, a);
            if (is(e, "atoms_replaced") || is(e, "box_changed")) CHECK(!h.frc_valid() && !h.reusable_run_forces(), "%s from %04x: %04x", e.name, b, a);
            // 4.
            if (is(e, "coords_written")) CHECK(!h.frc_valid() && h.state_set() && (h.stale() || h.coords_moved()) && !h.reusable_run_forces(), "%s from %04x: %04x", e.name, b, a);
            // 6.
            CHECK(!(off & A), "%s from %04x cleared params_set", e.name, b);
            if (off & C) CHECK(is(e, "box_changed"), "%s from %04x cleared state_set", e.name, b);
            // 7.
            if (on & P) CHECK(is(e, "state_write_begins") && !(b & W) && (b & F), "%s from %04x set frc_before_set_state", e.name, b);
            // a comparison always closes the write it belongs to; a search, a prune, a drift leave what a setter is owed alone
            if (is(e, "state_compared")) CHECK(!h.state_pending() && !h.frc_before_set_state(), "%s from %04x: %04x", e.name, b, a);
            // every event is idempotent: a call site reached twice in a row changes nothing the second time
            { Held twice = h; e.apply(twice); CHECK(twice.bits() == a, "%s from %04x: second call %04x -> %04x", e.name, b, a, twice.bits()); }
        }
    }
    std::printf("sweep: %u states x %d events = %lld transitions\n", ALL + 1, n_events, n);
}

int main() {
    known_answers();
    std::printf("known answers: %d transitions of %d events\n", n_known, n_events);
    sweep();
    std::printf(failures ? "%d FAILURES\n" : "held_check: all passed\n", failures);
    return failures ? 1 : 0;
}
