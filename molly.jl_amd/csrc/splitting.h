// splitting.h — the plan of one LangevinSplitting step (simulators.jl:1269-1380): which sub-step runs with which time step, which B computes forces,
// and how the sub-steps fall into launches.  Host-only arithmetic on plain values: no HIP header, nothing of the engine
// (tests/host/splitting_check.cpp runs it alone), no state, no allocation, everything by value.
//
//   ops        the characters of the string, A (drift) | B (kick) | O (friction + noise), each with dt / count(op, string)          :1305
//   force flag forces_known starts true unless the string matches ^.*B[^B]*A[^B]*$ (an A behind the last B: the forces the step ends with belong
//              to coordinates that have moved on); an A clears it; a B that finds it cleared computes the forces and sets it            :1308-1324
//              — decided once per string, not per step
//   segments   a maximal run of sub-steps that ends in front of a force-computing B or at the end of the step: one launch of
//              k_split_segment (splitting.hip) each; a force pass sits in front of every segment that opens with such a B.  Never across a step
//              boundary: the centre-of-mass removal, the coupling and the neighbour cadence sit there.
// The reference takes a string of any length; the engine's program travels in the kernel arguments and holds SPLIT_MAX_OPS sub-steps.
#pragma once
#include <cstdint>

namespace mhip {

constexpr int SPLIT_MAX_OPS = 16;
enum SplitOp : int32_t { SPLIT_A = 0, SPLIT_B = 1, SPLIT_O = 2, SPLIT_OVERDAMPED = 3 };      // (the last: the whole OverdampedLangevin update, simulators.jl:1465-1466; never in a string)

struct SplitStep {
    int32_t op = SPLIT_A;
    double dt_eff = 0;              // dt / count(op, string)
    bool computes_forces = false;   // a B that finds the forces out of date
    int o_index = -1;               // an O: its number among the step's O sub-steps, 0-based (its Philox counter is ctr1 + o_index)
};
struct SplitSegment {
    int begin = 0, end = 0;         // ops[begin, end)
    bool forces_first = false;      // ops[begin] is a force-computing B: a force pass in front of the launch
    bool has_a = false, has_b = false, has_o = false;
};
struct SplitPlan {
    bool ok = false;                // false: null, empty, longer than SPLIT_MAX_OPS, or a character other than A, B, O
    int n_ops = 0;
    SplitStep ops[SPLIT_MAX_OPS];
    int n_a = 0, n_b = 0, n_o = 0;
    bool forces_known_at_start = true;
    int n_force = 0;                // force-computing B per step
    int n_seg = 0;
    SplitSegment seg[SPLIT_MAX_OPS];
};

inline SplitPlan plan_splitting(const char* s, double dt) {
    SplitPlan p;
    if (!s) return p;
    int n = 0;
    while (n <= SPLIT_MAX_OPS && s[n] != '\0') ++n;
    if (n < 1 || n > SPLIT_MAX_OPS) return p;
    for (int j = 0; j < n; ++j) {
        if (s[j] == 'A') { p.ops[j].op = SPLIT_A; ++p.n_a; }
        else if (s[j] == 'B') { p.ops[j].op = SPLIT_B; ++p.n_b; }
        else if (s[j] == 'O') { p.ops[j].op = SPLIT_O; p.ops[j].o_index = p.n_o++; }
        else return p;
    }
    p.n_ops = n;
    for (int j = 0; j < n; ++j) p.ops[j].dt_eff = dt / (p.ops[j].op == SPLIT_A ? p.n_a : p.ops[j].op == SPLIT_B ? p.n_b : p.n_o);      // :1305
    // ^.*B[^B]*A[^B]*$ : there is a B, and an A somewhere behind the last one                                                         :1308
    int last_b = -1;
    for (int j = 0; j < n; ++j) if (p.ops[j].op == SPLIT_B) last_b = j;
    bool a_behind = false;
    for (int j = last_b + 1; last_b >= 0 && j < n; ++j) a_behind = a_behind || p.ops[j].op == SPLIT_A;
    p.forces_known_at_start = !a_behind;
    bool known = p.forces_known_at_start;
    for (int j = 0; j < n; ++j) {                                                                                                       // :1310-1324
        if (p.ops[j].op == SPLIT_A) known = false;
        else if (p.ops[j].op == SPLIT_B && !known) { p.ops[j].computes_forces = true; known = true; ++p.n_force; }
    }
    for (int j = 0; j < n; ++j) {
        if (j == 0 || p.ops[j].computes_forces) { SplitSegment& g = p.seg[p.n_seg++]; g.begin = j; g.forces_first = p.ops[j].computes_forces; }
        SplitSegment& g = p.seg[p.n_seg - 1];
        g.end = j + 1;
        g.has_a = g.has_a || p.ops[j].op == SPLIT_A; g.has_b = g.has_b || p.ops[j].op == SPLIT_B; g.has_o = g.has_o || p.ops[j].op == SPLIT_O;
    }
    p.ok = true;
    return p;
}

}  // namespace mhip
