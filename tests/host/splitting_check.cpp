// splitting_check — prints plan_splitting (molly.jl_amd/csrc/splitting.h) for every string over {A, B, O} of length 1 to 6 and for the inputs it must reject;
// tests/test_splitting_host.py compares the lines with the reference's rule restated in Python (tests/splitting_ref.py).  Host-only: nothing but the header.
//   ok <string> known=<0|1> n_o=<n> n_force=<n> dts=<dt_eff,…> force=<0|1,…> oidx=<k|-,…> seg=<begin>-<end>:<forces_first><a><b><o>,…
//   bad <label>
#include <cstdio>
#include <string>

#include "splitting.h"

static void show(const std::string& s, double dt) {
    const mhip::SplitPlan p = mhip::plan_splitting(s.c_str(), dt);
    if (!p.ok) { std::printf("bad %s\n", s.c_str()); return; }
    std::printf("ok %s known=%d n_o=%d n_force=%d dts=", s.c_str(), p.forces_known_at_start ? 1 : 0, p.n_o, p.n_force);
    for (int j = 0; j < p.n_ops; ++j) std::printf("%s%.17g", j ? "," : "", p.ops[j].dt_eff);
    std::printf(" force=");
    for (int j = 0; j < p.n_ops; ++j) std::printf("%s%d", j ? "," : "", p.ops[j].computes_forces ? 1 : 0);
    std::printf(" oidx=");
    for (int j = 0; j < p.n_ops; ++j) { if (p.ops[j].o_index < 0) std::printf("%s-", j ? "," : ""); else std::printf("%s%d", j ? "," : "", p.ops[j].o_index); }
    std::printf(" seg=");
    for (int g = 0; g < p.n_seg; ++g)
        std::printf("%s%d-%d:%d%d%d%d", g ? "," : "", p.seg[g].begin, p.seg[g].end, p.seg[g].forces_first ? 1 : 0, p.seg[g].has_a ? 1 : 0, p.seg[g].has_b ? 1 : 0, p.seg[g].has_o ? 1 : 0);
    std::printf("\n");
}

int main() {
    const double dt = 0.002;
    const char abc[3] = {'A', 'B', 'O'};
    int n = 0;
    for (int len = 1; len <= 6; ++len) {
        int total = 1;
        for (int k = 0; k < len; ++k) total *= 3;
        for (int code = 0; code < total; ++code) {
            std::string s;
            for (int k = 0, c = code; k < len; ++k, c /= 3) s.push_back(abc[c % 3]);
            show(s, dt); ++n;
        }
    }
    std::printf("strings: %d\n", n);
    show("BAOABBAOABBAOABB", dt);      // 16 sub-steps: the longest program
    std::printf("%s null\n", mhip::plan_splitting(nullptr, dt).ok ? "ok" : "bad");
    std::printf("%s empty\n", mhip::plan_splitting("", dt).ok ? "ok" : "bad");
    std::printf("%s seventeen\n", mhip::plan_splitting("BAOABBAOABBAOABBA", dt).ok ? "ok" : "bad");
    std::printf("%s lowercase\n", mhip::plan_splitting("BAoAB", dt).ok ? "ok" : "bad");
    std::printf("%s other\n", mhip::plan_splitting("BAXAB", dt).ok ? "ok" : "bad");
    return 0;
}
