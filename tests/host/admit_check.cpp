// Stand-alone check of molly.jl_amd/csrc/admit.h (tests/test_admit_host.py compiles and runs it): known answers — for every entry the state that
// holds exactly its needs, that state with each single mode added and with each single need removed, written down by hand from the header's
// table — then a sweep over every mode combination × every entry for the properties the header lists.  Exit status 0 = pass.
#include <cstdio>
#include <cstring>
#include <vector>

#include "admit.h"

using namespace mhip::adm;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; if (failures < 50) { std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// The table of the header, transcribed by hand: one character per column, in the order of the bits.
//   .  not read     U / S  refused with that code when on     s  refused with STATE when missing     g  refused with UNSUPPORTED when on next to GHOSTS
//                                STATE PARAMS GHOSTS DOMAIN_PLAN PEERS TRICLINIC CONSTRAINTS SITES THERMOSTAT ANDERSEN HALO_PLAN ROUTES REGION PEERS_OPEN FORCES PME EXCEPTIONS CALLER_TOPOLOGY
struct Expect { Entry e; const char* cells; };
static const Expect table[] = {
    {VV_RUN,            "ssS..............."},
    {LANGEVIN_RUN,      "ssS.....U........."},
    {VV_INIT,           "s.....UU.........."},
    {VV_STAGE1,         "......UUU.....s..."},
    {VV_STAGE2,         "......UUU........."},
    {HALO_START,        "......UUU.s...s..."},
    {HALO_MID,          "......UUU.s......."},
    {HALO_BEGIN,        "......UUU.....s..."},
    {HALO_END,          "......UUU........."},
    {HALO_END_PARTS,    "......UUU........."},
    {DOMAIN_RUN,        "......UUU.ss..s..."},
    {REDRAW,            "ssU..............."},
    {TUNE,              "ssU..............."},
    {SET_BOX,           "..UUU............."},
    {CONSTRAINT_VIRIAL, "ss................"},
    {PLACE_SITES,       "s................."},
    {DISTRIBUTE_FORCES, "s................."},
    {SPECIFIC_FORCES,   "s................."},
    {SPECIFIC_VIRIAL,   "s................."},
    {SPECIFIC_ENERGY,   "s................."},
    {GENERAL_FORCES,    "s................."},
    {GENERAL_VIRIAL,    "s................."},
    {GENERAL_ENERGY,    "s................."},
    {SET_ROUTES,        "..........s.s....."},
    {OPEN_PEER,         "............s....."},
    {SELFTEST,          "............ss...."},
    {DOMAIN_EXPORT,     "...s.............."},
    {ON_GHOSTS,         ".....UUUU........."},
    {ON_DOMAIN_PLAN,    "......UUU........U"},
    {ON_PEERS,          "......UUU........."},
    {ON_TRICLINIC,      "..U...UU.........."},
    {ON_CONSTRAINTS,    "..UUUU...UU......."},
    {ON_SITES,          "..UUUU...UU......."},
    {ON_THERMOSTAT,     "..UUU....UU......."},
    {ON_ANDERSEN,       "......UUU........."},
    {ON_HALO_PLAN,      "......UUU........."},
    {SEARCH,            "ss..............g."},
    {FORCE_PASS,        "...............g.."},
};
static const int n_entries = (int)(sizeof(table) / sizeof(table[0]));
static const uint32_t ALL = (1u << N_MODES) - 1;

static uint32_t cells_of(const Expect& x, const char* kinds) {
    uint32_t m = 0;
    for (int k = 0; k < N_MODES; ++k) if (std::strchr(kinds, x.cells[k])) m |= 1u << k;
    return m;
}
static const char* code_name(Code c) { return c == Code::OK ? "OK" : c == Code::UNSUPPORTED ? "UNSUPPORTED" : "STATE"; }

static int n_known = 0;
static void known(Entry e, uint32_t modes, Code want) {
    const Verdict v = admit(e, modes);
    ++n_known;
    CHECK(v.code == want, "%s at %05x: %s, expected %s", row(e).name, modes, code_name(v.code), code_name(want));
    CHECK(v.why != nullptr && ((v.code == Code::OK) == (v.why[0] == 0)), "%s at %05x: the sentence", row(e).name, modes);
}
static void known_answers() {
    CHECK(n_entries == N_ENTRIES, "%d rows for %d entries", n_entries, (int)N_ENTRIES);
    for (int i = 0; i < n_entries; ++i) {
        const Expect& x = table[i];
        CHECK((int)x.e == i && std::strlen(x.cells) == (size_t)N_MODES, "row %d", i);
        const uint32_t needs = cells_of(x, "s");
        known(x.e, needs, Code::OK);
        for (int k = 0; k < N_MODES; ++k) {
            const uint32_t m = 1u << k;
            if (needs & m) { known(x.e, needs & ~m, Code::STATE); continue; }
            const char c = x.cells[k];
            known(x.e, needs | m, c == 'U' ? Code::UNSUPPORTED : c == 'S' ? Code::STATE : Code::OK);
            if (c == 'g') known(x.e, needs | m | GHOSTS, Code::UNSUPPORTED);
        }
    }
    // a few written out in full.  The closing kick of a constrained context has no RATTLE: halo_end refuses it
    known(HALO_END, STATE | PARAMS | FORCES | CONSTRAINTS, Code::UNSUPPORTED);
    known(HALO_END_PARTS, STATE | PARAMS | SITES, Code::UNSUPPORTED);
    known(VV_RUN, STATE | PARAMS | CONSTRAINTS | SITES | THERMOSTAT | DOMAIN_PLAN | HALO_PLAN | FORCES | PME | CALLER_TOPOLOGY, Code::OK);
    known(LANGEVIN_RUN, STATE | PARAMS | CONSTRAINTS | SITES | ANDERSEN, Code::OK);
    known(ON_CONSTRAINTS, HALO_PLAN, Code::UNSUPPORTED);
    known(ON_HALO_PLAN, SITES, Code::UNSUPPORTED);
    known(ON_PEERS, THERMOSTAT, Code::UNSUPPORTED);
    known(ON_TRICLINIC, DOMAIN_PLAN | HALO_PLAN | PEERS | THERMOSTAT | ANDERSEN, Code::OK);      // (not widened to the rest of the multi-domain class)
    // the first refusing column from the left decides
    known(VV_RUN, GHOSTS, Code::STATE);                                         // no coordinates (needed) before the ghosts
    known(LANGEVIN_RUN, STATE | PARAMS | GHOSTS | THERMOSTAT, Code::STATE);     // ghosts (STATE) before the thermostat (UNSUPPORTED)
    known(HALO_START, CONSTRAINTS, Code::UNSUPPORTED);                          // constraints before the missing plan
    known(HALO_START, 0, Code::STATE);
    known(TUNE, GHOSTS, Code::STATE);
    known(TUNE, STATE | PARAMS | GHOSTS, Code::UNSUPPORTED);
}

// the excluded pairs (rule 2), and the entry that turns each mode on
struct TurnOn { uint32_t mode; Entry e; };
static const TurnOn turn_on[] = {{GHOSTS, ON_GHOSTS}, {DOMAIN_PLAN, ON_DOMAIN_PLAN}, {PEERS, ON_PEERS}, {TRICLINIC, ON_TRICLINIC}, {CONSTRAINTS, ON_CONSTRAINTS},
                                 {SITES, ON_SITES}, {THERMOSTAT, ON_THERMOSTAT}, {ANDERSEN, ON_ANDERSEN}, {HALO_PLAN, ON_HALO_PLAN}};
static const int n_turn_on = (int)(sizeof(turn_on) / sizeof(turn_on[0]));
static Entry on_entry(uint32_t mode) { for (const TurnOn& t : turn_on) if (t.mode == mode) return t.e; return N_ENTRIES; }
struct Pair { uint32_t a, b; };
static std::vector<Pair> excluded_pairs() {
    std::vector<Pair> p;
    for (uint32_t f : {CONSTRAINTS, SITES, THERMOSTAT}) for (uint32_t m : {GHOSTS, DOMAIN_PLAN, HALO_PLAN, PEERS}) p.push_back({f, m});
    p.push_back({TRICLINIC, GHOSTS});
    for (uint32_t f : {CONSTRAINTS, SITES}) p.push_back({TRICLINIC, f});
    for (uint32_t f : {CONSTRAINTS, SITES, THERMOSTAT}) p.push_back({ANDERSEN, f});
    return p;
}
static bool has_excluded_pair(uint32_t s, const std::vector<Pair>& pairs) {
    for (const Pair& p : pairs) if ((s & p.a) && (s & p.b)) return true;
    return false;
}

static void sweep() {
    const std::vector<Pair> pairs = excluded_pairs();
    CHECK(pairs.size() == 18, "%d pairs", (int)pairs.size());
    // 1. the entries that launch an integrator but not k_con_step, and those besides VV_RUN that advance velocities
    const Entry plain_steppers[] = {VV_STAGE1, VV_STAGE2, HALO_START, HALO_MID, HALO_BEGIN, HALO_END, HALO_END_PARTS, DOMAIN_RUN};
    const Entry uncoupled[] = {LANGEVIN_RUN, VV_STAGE1, VV_STAGE2, HALO_START, HALO_MID, HALO_BEGIN, HALO_END, HALO_END_PARTS, DOMAIN_RUN};
    long long n = 0;
    for (uint32_t s = 0; s <= ALL; ++s) {
        for (int i = 0; i < n_entries; ++i) {
            const Expect& x = table[i];
            const Code c = admit(x.e, s).code;
            ++n;
            // 5. only the columns the row names (the 'g' cells read GHOSTS too)
            const uint32_t named = cells_of(x, "sUSg") | (cells_of(x, "g") ? (uint32_t)GHOSTS : 0u);
            CHECK(admit(x.e, s & named).code == c, "%s at %05x: reads a column its row does not name", row(x.e).name, s);
            // a refusal has a reason in the row: some refused column on, or some needed column missing
            const uint32_t needs = cells_of(x, "s"), refused = cells_of(x, "US") | ((s & GHOSTS) ? cells_of(x, "g") : 0u);
            CHECK((c != Code::OK) == ((s & refused) != 0 || (needs & ~s) != 0), "%s at %05x: %s", row(x.e).name, s, code_name(c));
        }
        // 1.
        if (s & (CONSTRAINTS | SITES)) for (Entry e : plain_steppers) CHECK(admit(e, s).code != Code::OK, "%s at %05x steps constraints / sites without k_con_step", row(e).name, s);
        if (s & THERMOSTAT) for (Entry e : uncoupled) CHECK(admit(e, s).code != Code::OK, "%s at %05x steps past a thermostat", row(e).name, s);
        // 2. both turn-on entries of an excluded pair refuse the other side
        for (const Pair& p : pairs) {
            if (s & p.b) CHECK(admit(on_entry(p.a), s).code == Code::UNSUPPORTED, "%s at %05x", row(on_entry(p.a)).name, s);
            if (s & p.a) CHECK(admit(on_entry(p.b), s).code == Code::UNSUPPORTED, "%s at %05x", row(on_entry(p.b)).name, s);
        }
    }
    // 4. no entry refuses the state in which only its needs are set
    for (int i = 0; i < n_entries; ++i) CHECK(admit(table[i].e, cells_of(table[i], "s")).code == Code::OK, "%s refuses its own needs", row(table[i].e).name);
    // 3. closure: from the empty context, through admitted turn-ons and any turn-off (what is present may come and go freely), no excluded pair is reached
    uint32_t settable = 0;
    for (const TurnOn& t : turn_on) settable |= t.mode;
    std::vector<char> seen(ALL + 1, 0);
    std::vector<uint32_t> todo{0u};
    seen[0] = 1;
    long long reached = 0;
    while (!todo.empty()) {
        const uint32_t s = todo.back(); todo.pop_back();
        ++reached;
        CHECK(!has_excluded_pair(s, pairs), "reachable state %05x holds an excluded pair", s);
        for (int k = 0; k < N_MODES; ++k) {
            const uint32_t m = 1u << k;
            uint32_t t = s ^ m;
            if ((settable & m) && !(s & m) && admit(on_entry(m), s).code != Code::OK) continue;      // a refused turn-on
            if (!seen[t]) { seen[t] = 1; todo.push_back(t); }
        }
    }
    // … and every state without an excluded pair is reachable: the exclusions are all that the turn-on entries refuse, CALLER_TOPOLOGY × DOMAIN_PLAN aside
    long long free_states = 0;
    for (uint32_t s = 0; s <= ALL; ++s) if (!has_excluded_pair(s, pairs)) { ++free_states; CHECK(seen[s], "state %05x holds no excluded pair and cannot be reached", s); }
    std::printf("sweep: %u states x %d entries = %lld verdicts; %lld states reachable of %lld without an excluded pair\n", ALL + 1, n_entries, n, reached, free_states);
}

int main() {
    known_answers();
    std::printf("known answers: %d verdicts of %d entries\n", n_known, n_entries);
    sweep();
    std::printf(failures ? "%d FAILURES\n" : "admit_check: all passed\n", failures);
    return failures ? 1 : 0;
}
