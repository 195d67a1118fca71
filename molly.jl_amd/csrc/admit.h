// admit.h — which call a context admits in its present configuration.  Host-only and pure: a bit set of modes describing the context, one
// entry per thing a caller can ask, one table.  No device code, nothing of the engine (tests/host/admit_check.cpp runs it alone).
//
// The engine forms the modes in ONE place (Engine::modes) and asks ONE question (Engine::admit(Entry)) at the top of every entry point, before
// any side effect; the helpers the step loops use (stage1_impl, init_impl, halo_mid_impl, …) ask nothing.  Argument validation (MHIP_ERR_INVALID)
// and the refusals that depend on the data handed over (an unhosted site, a brick that neighbours itself, …) stay with the entry points.
//
// This table is the rule (DESIGN.md §5b repeats it).  Rows: entries.  Columns: modes, in the order of their bits.
//   ·  the column is not read        U / S  refused with UNSUPPORTED / STATE when the mode is ON        s  refused with STATE when the mode is MISSING
//   u* refused with UNSUPPORTED when the mode is on TOGETHER with GHOSTS (the two lazy checks)
// When several cells refuse, the answer is that of the FIRST such column from the left.
//
//                    STATE PARAM GHOST DOMPL PEERS TRICL CONST SITES THERM ANDER HPLAN ROUTE REGIO POPEN FORCE  PME  EXCEP CTOPO
//   VV_RUN             s     s     S     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_vv_run
//   LANGEVIN_RUN       s     s     S     ·     ·     ·     ·     ·     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_langevin_run
//   VV_INIT            s     ·     ·     ·     ·     ·     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_vv_init
//   VV_STAGE1          ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     s     ·     ·     ·     mhip_vv_stage1
//   VV_STAGE2          ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_vv_stage2
//   HALO_START         ·     ·     ·     ·     ·     ·     U     U     U     ·     s     ·     ·     ·     s     ·     ·     ·     mhip_vv_halo_start
//   HALO_MID           ·     ·     ·     ·     ·     ·     U     U     U     ·     s     ·     ·     ·     ·     ·     ·     ·     mhip_vv_halo_mid
//   HALO_BEGIN         ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     s     ·     ·     ·     mhip_vv_halo_begin
//   HALO_END           ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_vv_halo_end
//   HALO_END_PARTS     ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_vv_halo_end_parts
//   DOMAIN_RUN         ·     ·     ·     ·     ·     ·     U     U     U     ·     s     s     ·     ·     s     ·     ·     ·     mhip_domain_run (a)
//   REDRAW             s     s     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_andersen, mhip_random_velocities
//   TUNE               s     s     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_tune_launch
//   SET_BOX            ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_set_box
//   CONSTRAINT_VIRIAL  s     s     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_constraint_virial (b)
//   PLACE_SITES        s     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_place_virtual_sites
//   DISTRIBUTE_FORCES  s     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_distribute_forces (b)
//   SPECIFIC_FORCES, SPECIFIC_VIRIAL, SPECIFIC_ENERGY, GENERAL_FORCES, GENERAL_VIRIAL, GENERAL_ENERGY: as PLACE_SITES (the coordinates)
//   SET_ROUTES         ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     s     ·     s     ·     ·     ·     ·     ·     mhip_set_halo_routes (c)
//   OPEN_PEER          ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     s     ·     ·     ·     ·     ·     mhip_halo_open_peer
//   SELFTEST           ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     s     s     ·     ·     ·     ·     mhip_halo_selftest
//   DOMAIN_EXPORT      ·     ·     ·     s     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_domain_export
//   -- the turn-on forms of the setters (turning a feature off is always admitted) --
//   ON_GHOSTS          ·     ·     ·     ·     ·     U     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_set_atom_counts, n_ghost > 0
//   ON_DOMAIN_PLAN     ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     U     mhip_set_domain, a geometry
//   ON_PEERS           ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_halo_region, world > 1
//   ON_TRICLINIC       ·     ·     U     ·     ·     ·     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_set_triclinic
//   ON_CONSTRAINTS     ·     ·     U     U     U     U     ·     ·     ·     U     U     ·     ·     ·     ·     ·     ·     ·     mhip_set_constraints, any constraint
//   ON_SITES           ·     ·     U     U     U     U     ·     ·     ·     U     U     ·     ·     ·     ·     ·     ·     ·     mhip_set_virtual_sites, any site
//   ON_THERMOSTAT      ·     ·     U     U     U     ·     ·     ·     ·     U     U     ·     ·     ·     ·     ·     ·     ·     mhip_set_thermostat, kind != off
//   ON_ANDERSEN        ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_set_andersen, prob > 0
//   ON_HALO_PLAN       ·     ·     ·     ·     ·     ·     U     U     U     ·     ·     ·     ·     ·     ·     ·     ·     ·     mhip_set_halo_plan, a plan
//   -- the two lazy checks, asked where the work is about to be done --
//   SEARCH             s     s     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     u*    ·     rebuild_impl: a pair-list search
//   FORCE_PASS         ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     ·     u*    ·     ·     step_forces, the PME launches (d)
//
//   (a) a run of no steps kicks nothing: the engine grants it FORCES; ROUTE stands for "routes set, or a plan that sends nothing" (one brick)
//   (b) asked only of a context that has constraints / sites (without them the call is a no-op); DISTRIBUTE_FORCES reads the coordinates for an
//       OutOfPlaneSite only: the engine grants STATE to a site set without one
//   (c) routes without peers need no region: the engine grants REGIO then
//   (d) the row reads nothing but PME next to GHOST: inside the step loops the engine asks it only of a context with ghosts
//
// What the table guarantees (swept over every mode combination × every entry by the host check):
//   1. an integrator that ignores a feature refuses it: every entry that launches an integrator but not k_con_step (all steppers except VV_RUN and
//      LANGEVIN_RUN) refuses CONST and SITES; every entry other than VV_RUN that advances velocities refuses THERM
//   2. exclusions are symmetric, so the order of two setters cannot matter: for every excluded pair both turn-on entries refuse the other side.
//      The pairs: {CONST, SITES, THERM} × {GHOST, DOMPL, HPLAN, PEERS};  TRICL × GHOST;  TRICL × {CONST, SITES};  ANDER × {CONST, SITES, THERM}
//   3. closure: from the empty context, through admitted turn-on entries and any turn-off, no state with an excluded pair is reached
//   4. no entry refuses a state in which only its needs are set
//   5. an entry's verdict depends only on the columns its row names
#pragma once
#include <cstdint>

namespace mhip {
namespace adm {

enum Mode : uint32_t {
    STATE = 1u << 0,             // coordinates have been handed over (held.state_set())
    PARAMS = 1u << 1,            // per-atom parameters have been handed over (held.params_set())
    GHOSTS = 1u << 2,            // n_ghost > 0
    DOMAIN_PLAN = 1u << 3,       // mhip_set_domain gave a geometry (dom.ready)
    PEERS = 1u << 4,             // mhip_halo_region with world > 1
    TRICLINIC = 1u << 5,
    CONSTRAINTS = 1u << 6,
    SITES = 1u << 7,
    THERMOSTAT = 1u << 8,        // a rescaling thermostat is set
    ANDERSEN = 1u << 9,          // the Andersen coupling is set (prob > 0)
    HALO_PLAN = 1u << 10,        // mhip_set_halo_plan gave a plan
    ROUTES = 1u << 11,           // mhip_set_halo_routes gave routes (or the plan sends nothing)
    REGION = 1u << 12,           // mhip_halo_region allocated this rank's receive region
    PEERS_OPEN = 1u << 13,       // every rank's region is mapped
    FORCES = 1u << 14,           // the total force of the coordinates held is in place (held.frc_valid())
    PME = 1u << 15,
    EXCEPTIONS = 1u << 16,       // exception lists
    CALLER_TOPOLOGY = 1u << 17   // anything indexed by caller order: bonded terms, exceptions, special pairs, PME
};
constexpr int N_MODES = 18;

enum Entry : int {
    VV_RUN, LANGEVIN_RUN, VV_INIT, VV_STAGE1, VV_STAGE2, HALO_START, HALO_MID, HALO_BEGIN, HALO_END, HALO_END_PARTS, DOMAIN_RUN,
    REDRAW, TUNE, SET_BOX, CONSTRAINT_VIRIAL, PLACE_SITES, DISTRIBUTE_FORCES,
    SPECIFIC_FORCES, SPECIFIC_VIRIAL, SPECIFIC_ENERGY, GENERAL_FORCES, GENERAL_VIRIAL, GENERAL_ENERGY,
    SET_ROUTES, OPEN_PEER, SELFTEST, DOMAIN_EXPORT,
    ON_GHOSTS, ON_DOMAIN_PLAN, ON_PEERS, ON_TRICLINIC, ON_CONSTRAINTS, ON_SITES, ON_THERMOSTAT, ON_ANDERSEN, ON_HALO_PLAN,
    SEARCH, FORCE_PASS,
    N_ENTRIES
};

enum class Code { OK, UNSUPPORTED, STATE, N_CODES };      // (mapped to the MHIP_ERR_* codes in one place in engine.hip)
struct Verdict { Code code; const char* why; };

// one row of the table: the columns refused with UNSUPPORTED / STATE when on, refused with STATE when missing, refused with UNSUPPORTED next to GHOSTS
struct Row { const char* name; uint32_t off_u, off_s, need, with_ghosts; };

inline const Row& row(Entry e) {
    constexpr uint32_t FEATURES = CONSTRAINTS | SITES | THERMOSTAT, MULTI = GHOSTS | DOMAIN_PLAN | PEERS | HALO_PLAN;
    static const Row rows[N_ENTRIES] = {
        {"mhip_vv_run", 0, GHOSTS, STATE | PARAMS, 0},
        {"mhip_langevin_run", THERMOSTAT, GHOSTS, STATE | PARAMS, 0},
        {"mhip_vv_init", CONSTRAINTS | SITES, 0, STATE, 0},
        {"mhip_vv_stage1", FEATURES, 0, FORCES, 0},
        {"mhip_vv_stage2", FEATURES, 0, 0, 0},
        {"mhip_vv_halo_start", FEATURES, 0, HALO_PLAN | FORCES, 0},
        {"mhip_vv_halo_mid", FEATURES, 0, HALO_PLAN, 0},
        {"mhip_vv_halo_begin", FEATURES, 0, FORCES, 0},
        {"mhip_vv_halo_end", FEATURES, 0, 0, 0},
        {"mhip_vv_halo_end_parts", FEATURES, 0, 0, 0},
        {"mhip_domain_run", FEATURES, 0, HALO_PLAN | ROUTES | FORCES, 0},
        {"a velocity draw", GHOSTS, 0, STATE | PARAMS, 0},
        {"mhip_tune_launch", GHOSTS, 0, STATE | PARAMS, 0},
        {"mhip_set_box", GHOSTS | DOMAIN_PLAN | PEERS, 0, 0, 0},
        {"mhip_constraint_virial", 0, 0, STATE | PARAMS, 0},
        {"mhip_place_virtual_sites", 0, 0, STATE, 0},
        {"mhip_distribute_forces", 0, 0, STATE, 0},
        {"mhip_specific_forces", 0, 0, STATE, 0},
        {"mhip_specific_virial", 0, 0, STATE, 0},
        {"mhip_specific_potential_energy", 0, 0, STATE, 0},
        {"mhip_general_forces", 0, 0, STATE, 0},
        {"mhip_general_virial", 0, 0, STATE, 0},
        {"mhip_general_potential_energy", 0, 0, STATE, 0},
        {"mhip_set_halo_routes", 0, 0, HALO_PLAN | REGION, 0},
        {"mhip_halo_open_peer", 0, 0, REGION, 0},
        {"mhip_halo_selftest", 0, 0, REGION | PEERS_OPEN, 0},
        {"mhip_domain_export", 0, 0, DOMAIN_PLAN, 0},
        {"mhip_set_atom_counts with ghosts", TRICLINIC | FEATURES, 0, 0, 0},
        {"mhip_set_domain", FEATURES | CALLER_TOPOLOGY, 0, 0, 0},
        {"mhip_halo_region with peers", FEATURES, 0, 0, 0},
        {"mhip_set_triclinic", GHOSTS | CONSTRAINTS | SITES, 0, 0, 0},
        {"mhip_set_constraints", MULTI | TRICLINIC | ANDERSEN, 0, 0, 0},
        {"mhip_set_virtual_sites", MULTI | TRICLINIC | ANDERSEN, 0, 0, 0},
        {"mhip_set_thermostat", MULTI | ANDERSEN, 0, 0, 0},
        {"mhip_set_andersen", FEATURES, 0, 0, 0},
        {"mhip_set_halo_plan", FEATURES, 0, 0, 0},
        {"a pair-list search", 0, 0, STATE | PARAMS, EXCEPTIONS},
        {"a force pass", 0, 0, 0, PME},
    };
    return rows[e];
}

// one sentence per (column, reason); the entry's name in front of it makes the message
inline const char* why_on(uint32_t mode) {
    switch (mode) {
        case GHOSTS: return "runs on a single domain, and this context has ghost atoms";
        case DOMAIN_PLAN: return "runs on a single domain, and this context has a domain plan (mhip_set_domain)";
        case PEERS: return "runs on a single domain, and this context has peers (mhip_halo_region)";
        case HALO_PLAN: return "runs on a single domain, and this context has a halo plan (mhip_set_halo_plan)";
        case TRICLINIC: return "is not supported with a TriclinicBoundary";
        case CONSTRAINTS: return "is not available to a context with constraints: they run on a single domain with a rectangular box, stepped by mhip_vv_run / mhip_langevin_run, without the Andersen coupling";
        case SITES: return "is not available to a context with virtual sites: they run on a single domain with a rectangular box, stepped by mhip_vv_run / mhip_langevin_run, without the Andersen coupling";
        case THERMOSTAT: return "is not available to a context with a rescaling thermostat: those run on a single domain, stepped by mhip_vv_run, without the Andersen coupling";
        case ANDERSEN: return "is not supported next to the Andersen coupling";
        case CALLER_TOPOLOGY: return "moves atoms between ranks and resets the caller order: contexts with bonded terms, exception lists, special pairs or PME keep the host planner";
        case EXCEPTIONS: return "does not support exception lists with ghost atoms";
        case PME: return "runs PME on a single domain only";
    }
    return "is not supported in this configuration";
}
inline const char* why_missing(uint32_t mode) {
    switch (mode) {
        case STATE: return "needs coordinates: mhip_set_state first";
        case PARAMS: return "needs the atoms' parameters: mhip_set_atoms first";
        case DOMAIN_PLAN: return "needs a domain plan: mhip_set_domain first";
        case HALO_PLAN: return "needs a halo plan: mhip_set_halo_plan first";
        case ROUTES: return "needs routes: mhip_set_halo_routes first";
        case REGION: return "needs this rank's region: mhip_halo_region first";
        case PEERS_OPEN: return "needs every rank's region: mhip_halo_open_peer for every rank first";
        case FORCES: return "needs the forces of the coordinates held: mhip_vv_init / a finished step first";
    }
    return "is called out of order";
}

inline Verdict admit(Entry e, uint32_t modes) {
    const Row& r = row(e);
    const uint32_t pair = (modes & GHOSTS) ? r.with_ghosts : 0u;
    for (uint32_t m = 1u; m < (1u << N_MODES); m <<= 1) {      // the first refusing column from the left
        if (modes & m) {
            if ((r.off_u | pair) & m) return {Code::UNSUPPORTED, why_on(m)};
            if (r.off_s & m) return {Code::STATE, why_on(m)};
        } else if (r.need & m) return {Code::STATE, why_missing(m)};
    }
    return {Code::OK, ""};
}

}  // namespace adm
}  // namespace mhip
