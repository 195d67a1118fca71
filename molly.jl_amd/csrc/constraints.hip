// constraints.hip — SHAKE / RATTLE clusters and the constrained integrator launch (see constraints.h)
#include "constraints.h"

#include <algorithm>
#include <numeric>

#include "integrate.h"
#include "philox.h"

namespace mhip {

// ---- host: clusters (constraints.jl:251-344) ---------------------------------------------------------------------------------------
ClusterSet build_clusters(int64_t n_atoms, int64_t n_dist, const int32_t* ci, const int32_t* cj, const double* dist,
                          int64_t n_angle, const int32_t* ai, const int32_t* aj, const int32_t* ak, const double* d3, const SiteSet* vs) {
    auto bad = [](const std::string& m) { return ApiError{MHIP_ERR_INVALID, "constraints: " + m}; };
    if (n_dist < 0 || n_angle < 0) throw bad("negative count");
    if (n_dist > 0 && (!ci || !cj || !dist)) throw bad("null distance-constraint array");
    if (n_angle > 0 && (!ai || !aj || !ak || !d3)) throw bad("null angle-constraint array");
    auto in_range = [&](int32_t a) { return a >= 0 && (int64_t)a < n_atoms; };
    auto length_ok = [](double d) { return d > 0 && std::isfinite(d); };
    ClusterSet cs;
    std::vector<int32_t> owner((size_t)n_atoms, -1);      // cluster of an atom (central-atom clusters: index of the component's root)
    // central-atom clusters: the connected components of the distance constraints, each a star of 1..3 edges
    std::vector<int32_t> parent((size_t)n_atoms);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int32_t a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
    for (int64_t c = 0; c < n_dist; ++c) {
        if (!in_range(ci[c]) || !in_range(cj[c])) throw bad("atom index out of range in distance constraint " + std::to_string(c));
        if (ci[c] == cj[c]) throw bad("distance constraint " + std::to_string(c) + " joins an atom to itself");
        if (!length_ok(dist[c])) throw bad("distance constraint " + std::to_string(c) + " has a non-positive length");
        parent[find(ci[c])] = find(cj[c]);
    }
    std::vector<std::vector<int64_t>> comp_edges;
    std::vector<int32_t> comp_of((size_t)n_atoms, -1);
    for (int64_t c = 0; c < n_dist; ++c) {
        const int32_t r = find(ci[c]);
        if (comp_of[r] < 0) { comp_of[r] = (int32_t)comp_edges.size(); comp_edges.emplace_back(); }
        comp_edges[comp_of[r]].push_back(c);
    }
    struct Cl { int kind; int32_t a[4]; double d[3]; };
    std::vector<Cl> cls[4];
    for (size_t q = 0; q < comp_edges.size(); ++q) {
        const auto& e = comp_edges[q];
        const std::string where = "the cluster of atom " + std::to_string(ci[e[0]]);
        if (e.size() > 3) throw bad(where + " has " + std::to_string(e.size()) + " constraints (at most three on one central atom)");
        int32_t centre = ci[e[0]];
        if (e.size() > 1) {      // the atom every constraint shares
            const int32_t c0[2] = {ci[e[0]], cj[e[0]]};
            centre = -1;
            for (int32_t cand : c0) {
                bool all = true;
                for (int64_t c : e) all = all && (ci[c] == cand || cj[c] == cand);
                if (all) centre = cand;
            }
            if (centre < 0) throw bad(where + " is a chain or a ring (no central atom shared by all its constraints)");
        }
        Cl cl{}; cl.kind = (int)e.size() - 1; cl.a[0] = centre; cl.a[1] = cl.a[2] = cl.a[3] = -1;
        for (size_t k = 0; k < e.size(); ++k) {
            const int32_t other = ci[e[k]] == centre ? cj[e[k]] : ci[e[k]];
            for (size_t m = 1; m <= k; ++m)
                if (cl.a[m] == other) throw bad(where + " constrains the same pair twice");
            cl.a[k + 1] = other; cl.d[k] = dist[e[k]];
        }
        for (size_t k = 0; k <= e.size(); ++k) owner[cl.a[k]] = (int32_t)q;
        cls[cl.kind].push_back(cl);
    }
    // angle clusters: a triangle of their own, sharing no atom with any other cluster
    for (int64_t c = 0; c < n_angle; ++c) {
        const int32_t a[3] = {ai[c], aj[c], ak[c]};
        const double* d = d3 + 3 * c;
        for (int32_t x : a)
            if (!in_range(x)) throw bad("atom index out of range in angle constraint " + std::to_string(c));
        if (a[0] == a[1] || a[1] == a[2] || a[0] == a[2]) throw bad("angle constraint " + std::to_string(c) + " repeats an atom");
        for (int k = 0; k < 3; ++k)
            if (!length_ok(d[k])) throw bad("angle constraint " + std::to_string(c) + " has a non-positive length");
        for (int32_t x : a)
            if (owner[x] != -1) throw bad("atom " + std::to_string(x) + " is in two clusters (angle constraint " + std::to_string(c) + ")");
        // d = (d_ij, d_jk, d_ik): a linear (or impossible) triangle has no rigid shape SHAKE can hold
        const double s[3] = {d[0], d[1], d[2]};
        const double sum = s[0] + s[1] + s[2];
        if (std::min({s[0] + s[1] - s[2], s[1] + s[2] - s[0], s[0] + s[2] - s[1]}) <= 1e-6 * sum)
            throw bad("angle constraint " + std::to_string(c) + " is linear");
        for (int32_t x : a) owner[x] = -2;
        Cl cl{}; cl.kind = CK_ANGLE; cl.a[0] = a[0]; cl.a[1] = a[1]; cl.a[2] = a[2]; cl.a[3] = -1; cl.d[0] = d[0]; cl.d[1] = d[1]; cl.d[2] = d[2];
        cls[CK_ANGLE].push_back(cl);
    }
    // virtual sites: which item owns all the parents of each (constraints.h)
    const bool sites = vs && vs->n > 0;
    struct Host { int32_t type, site, l[3]; const double* w; };
    std::vector<std::vector<Host>> hosts[CK_N];
    for (int k = 0; k < 4; ++k) hosts[k].resize(cls[k].size());
    std::vector<int32_t> group((size_t)(sites ? n_atoms : 0));      // union of the free parents
    std::vector<std::vector<int32_t>> members;                       // … and the atoms of each union, ascending
    std::vector<int32_t> group_no((size_t)(sites ? n_atoms : 0), -1);
    if (sites) {
        for (int64_t a = 0; a < n_atoms; ++a)
            if (vs->flag[a] && owner[a] != -1) throw bad("atom " + std::to_string(a) + " is a virtual site but is also in a constraint");
        std::vector<int32_t> it_kind((size_t)n_atoms, -1), it_idx((size_t)n_atoms, -1), it_loc((size_t)n_atoms, -1);
        for (int k = 0; k < 4; ++k)
            for (size_t q = 0; q < cls[k].size(); ++q)
                for (int m = 0; m < 4; ++m)
                    if (cls[k][q].a[m] >= 0) { it_kind[cls[k][q].a[m]] = k; it_idx[cls[k][q].a[m]] = (int32_t)q; it_loc[cls[k][q].a[m]] = m; }
        std::iota(group.begin(), group.end(), 0);
        auto gfind = [&](int32_t a) { while (group[a] != a) { group[a] = group[group[a]]; a = group[a]; } return a; };
        auto unhosted = [&](int64_t s) { if (cs.first_unhosted < 0 || s < cs.first_unhosted) cs.first_unhosted = s; };
        std::vector<int8_t> where((size_t)vs->n, 0);                 // 1: a cluster hosts it, 2: its parents are free, 0: nobody can
        for (int64_t s = 0; s < vs->n; ++s) {
            const int32_t par[3] = {vs->a1[s], vs->a2[s], vs->a3[s]};
            int n_in = 0, n_free = 0, np = 0; bool same = true;
            for (int32_t x : par) {
                if (x < 0) continue;
                ++np;
                if (it_kind[x] >= 0) { ++n_in; same = same && it_kind[x] == it_kind[par[0]] && it_idx[x] == it_idx[par[0]]; } else ++n_free;
            }
            if (n_in == np && same) {
                Host h{vs->type[s], vs->site[s], {0, 0, 0}, vs->w.data() + 6 * s};
                for (int m = 0; m < 3; ++m) h.l[m] = par[m] >= 0 ? it_loc[par[m]] : 0;
                hosts[it_kind[par[0]]][it_idx[par[0]]].push_back(h);
                where[s] = 1;
            } else if (n_free == np) {
                for (int m = 1; m < 3; ++m) if (par[m] >= 0) group[gfind(par[m])] = gfind(par[0]);
                where[s] = 2;
            } else unhosted(s);
        }
        for (int64_t s = 0; s < vs->n; ++s) {
            if (where[s] != 2) continue;
            for (int32_t x : {vs->a1[s], vs->a2[s], vs->a3[s]})
                if (x >= 0 && group_no[gfind(x)] < 0) { group_no[gfind(x)] = (int32_t)members.size(); members.emplace_back(); }
        }
        for (int64_t a = 0; a < n_atoms; ++a) {                      // ascending: the local numbers follow the caller's order
            if (owner[a] != -1 || vs->flag[a]) continue;
            const int32_t g = group_no[gfind((int32_t)a)];
            if (g >= 0) { members[g].push_back((int32_t)a); group_no[a] = g; }
        }
        for (int k = CK_FREE; k < CK_N; ++k) hosts[k].resize(members.size());      // (indexed by union number; a union lands in one kind)
        for (int64_t s = 0; s < vs->n; ++s) {
            if (where[s] != 2) continue;
            const int32_t par[3] = {vs->a1[s], vs->a2[s], vs->a3[s]};
            const auto& mem = members[group_no[par[0]]];
            if (mem.size() > 4) { unhosted(s); continue; }
            Host h{vs->type[s], vs->site[s], {0, 0, 0}, vs->w.data() + 6 * s};
            for (int m = 0; m < 3; ++m) h.l[m] = par[m] >= 0 ? (int32_t)(std::find(mem.begin(), mem.end(), par[m]) - mem.begin()) : 0;
            hosts[mem.size() == 1 ? CK_FREE : CK_G2 + (int)mem.size() - 2][group_no[par[0]]].push_back(h);
        }
    }
    // layout: kind by kind, each padded to a whole wave, then the free atoms (then, with sites, the unconstrained groups)
    auto item = [&](const int32_t* a, const double* d, const std::vector<Host>* hs) {
        for (int m = 0; m < 4; ++m) { cs.atoms.push_back(a[m]); cs.d.push_back(m < 3 ? d[m] : 0.0); }
        if (!sites) return;
        cs.vs_item.push_back((int32_t)(cs.vs_rec.size() / 4)); cs.vs_item.push_back(hs ? (int32_t)hs->size() : 0);
        if (!hs || hs->empty()) return;
        ++cs.n_host_items; cs.n_hosted += (int64_t)hs->size();
        for (const Host& h : *hs) {
            cs.vs_rec.push_back(h.type); cs.vs_rec.push_back(h.site); cs.vs_rec.push_back(h.l[0] | (h.l[1] << 8) | (h.l[2] << 16)); cs.vs_rec.push_back(0);
            cs.vs_w.insert(cs.vs_w.end(), h.w, h.w + 6);
        }
    };
    const int32_t none4[4] = {-1, -1, -1, -1}; const double zero3[3] = {0, 0, 0};
    auto pad = [&]() { while (cs.atoms.size() % (4 * WAVE)) item(none4, zero3, nullptr); };
    for (int k = 0; k < 4; ++k) {
        for (size_t q = 0; q < cls[k].size(); ++q) {
            const Cl& cl = cls[k][q];
            const double d[3] = {cl.d[0], k == CK_2 ? 0.0 : cl.d[1], (k == CK_2 || k == CK_3) ? 0.0 : cl.d[2]};
            item(cl.a, d, sites ? &hosts[k][q] : nullptr);
        }
        pad();
        cs.end[k] = (int32_t)(cs.atoms.size() / 4);
        cs.n_kind[k] = (int64_t)cls[k].size();
    }
    for (int64_t a = 0; a < n_atoms; ++a) {
        if (owner[a] != -1 || (sites && vs->flag[a])) continue;      // (a site atom is nobody's work item: nothing integrates it)
        const int32_t g = sites ? group_no[a] : -1;
        if (g >= 0 && members[g].size() >= 2 && members[g].size() <= 4) continue;
        const int32_t one[4] = {(int32_t)a, -1, -1, -1};
        item(one, zero3, g >= 0 && members[g].size() == 1 ? &hosts[CK_FREE][g] : nullptr);
    }
    cs.end[CK_FREE] = (int32_t)(cs.atoms.size() / 4);
    for (int k = CK_G2; k < CK_N; ++k) {
        const size_t na = (size_t)(k - CK_G2 + 2);
        bool any = false;
        for (size_t g = 0; g < members.size(); ++g) {
            if (members[g].size() != na) continue;
            if (!any) {                                              // the free atoms, or the groups before, end on a whole wave
                const int32_t was = cs.end[k - 1];
                pad(); any = true;
                for (int j = k - 1; j >= CK_FREE && cs.end[j] == was; --j) cs.end[j] = (int32_t)(cs.atoms.size() / 4);
            }
            int32_t a4[4] = {-1, -1, -1, -1};
            for (size_t m = 0; m < na; ++m) a4[m] = members[g][m];
            item(a4, zero3, &hosts[k][g]);
            ++cs.n_groups;
        }
        cs.end[k] = (int32_t)(cs.atoms.size() / 4);
    }
    cs.n_constraints = n_dist + 3 * n_angle;
    return cs;
}

// ---- device --------------------------------------------------------------------------------------------------------------------------
namespace {

template <int K> struct Shape;
template <> struct Shape<CK_2> { static constexpr int NA = 2, NC = 1; };
template <> struct Shape<CK_3> { static constexpr int NA = 3, NC = 2; };
template <> struct Shape<CK_4> { static constexpr int NA = 4, NC = 3; };
template <> struct Shape<CK_ANGLE> { static constexpr int NA = 3, NC = 3; };
template <> struct Shape<CK_FREE> { static constexpr int NA = 1, NC = 0; };
template <> struct Shape<CK_G2> { static constexpr int NA = 2, NC = 0; };
template <> struct Shape<CK_G3> { static constexpr int NA = 3, NC = 0; };
template <> struct Shape<CK_G4> { static constexpr int NA = 4, NC = 0; };
// constraint c joins local atoms ca → cb (r = x_cb − x_ca): the centre to its c-th partner, or the triangle (0,1), (1,2), (0,2)
template <int K> __device__ constexpr int ca(int c) { return K == CK_ANGLE ? (c == 1 ? 1 : 0) : 0; }
template <int K> __device__ constexpr int cb(int c) { return K == CK_ANGLE ? (c == 0 ? 1 : 2) : c + 1; }
// ∂(x_cb − x_ca) / ∂g_e for a correction g_e·r_e/m on cb_e and −g_e·r_e/m on ca_e
template <int K> __device__ inline double kcoef(int c, int e, const double* im) {
    const int a = ca<K>(c), b = cb<K>(c), ae = ca<K>(e), be = cb<K>(e);
    return (double)((b == be) - (b == ae)) * im[b] - (double)((a == be) - (a == ae)) * im[a];
}
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// x ← A⁻¹ b, n <= 3, Gaussian elimination without pivoting: RATTLE's matrix is B M⁻¹ Bᵀ of the constraint gradients (symmetric positive definite),
// M-SHAKE's the same with one side taken at the start of the step — both diagonally dominant for the clusters build_clusters admits.  (Row swaps
// would index the registers at run time and put the matrix in scratch memory.)
template <int N> __device__ inline void solve(double (&A)[3][3], double (&b)[3]) {
#pragma unroll
    for (int p = 0; p < N; ++p) {
#pragma unroll
        for (int r = p + 1; r < N; ++r) {
            const double f = A[r][p] / A[p][p];
#pragma unroll
            for (int c = p; c < N; ++c) A[r][c] -= f * A[p][c];
            b[r] -= f * b[p];
        }
    }
#pragma unroll
    for (int p = N - 1; p >= 0; --p) {
        double s = b[p];
#pragma unroll
        for (int c = p + 1; c < N; ++c) s -= A[p][c] * b[c];
        b[p] = s / A[p][p];
    }
}

template <class T> __device__ inline void rel(const typename Vec<T>::T4& a, const typename Vec<T>::T4& b, const GridP<T>& G, double* r) {
    T dx, dy, dz;
    min_image_exact(a.x, a.y, a.z, b.x, b.y, b.z, G, dx, dy, dz);      // vector(a, b) = b − a, nearest image
    r[0] = dx; r[1] = dy; r[2] = dz;
}

// RATTLE (shake.jl:512-715): the velocities of the cluster with no component of any constrained pair's relative velocity along the
// pair, one linear solve
template <class T, int K> __device__ inline void rattle(const typename Vec<T>::T4* p, typename Vec<T>::T4* v, const double* im, const GridP<T>& G) {
    constexpr int NA = Shape<K>::NA, NC = Shape<K>::NC;
    double r[NC][3], A[3][3] = {}, b[3] = {};
#pragma unroll
    for (int c = 0; c < NC; ++c) rel<T>(p[ca<K>(c)], p[cb<K>(c)], G, r[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const auto &va = v[ca<K>(c)], &vb = v[cb<K>(c)];
        const double u[3] = {(double)vb.x - (double)va.x, (double)vb.y - (double)va.y, (double)vb.z - (double)va.z};
        b[c] = -dot3(r[c], u);
#pragma unroll
        for (int e = 0; e < NC; ++e) A[c][e] = kcoef<K>(c, e, im) * dot3(r[c], r[e]);
    }
    solve<NC>(A, b);
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        double dv[3] = {0, 0, 0};
#pragma unroll
        for (int e = 0; e < NC; ++e) {
            const double w = (double)((k == cb<K>(e)) - (k == ca<K>(e))) * b[e] * im[k];
            dv[0] += w * r[e][0]; dv[1] += w * r[e][1]; dv[2] += w * r[e][2];
        }
        v[k].x = (T)((double)v[k].x + dv[0]); v[k].y = (T)((double)v[k].y + dv[1]); v[k].z = (T)((double)v[k].z + dv[2]);
    }
}

// SHAKE: move the drifted positions p along the bonds of the start-of-step positions x0 until every constraint holds within tol.
// Two atoms: the smaller root of the quadratic (shake.jl:717-755); more: M-SHAKE, Newton steps on all constraints at once.
// Returns the iterations taken, negative when max_iters ran out first.
template <class T, int K> __device__ inline int shake(const typename Vec<T>::T4* x0, typename Vec<T>::T4* p, const double* im, const double* dl,
                                                      double tol, int max_iters, const GridP<T>& G) {
    constexpr int NA = Shape<K>::NA, NC = Shape<K>::NC;
    double r0[NC][3], q[NA][3], D[NA][3] = {}, g[NC] = {};
#pragma unroll
    for (int c = 0; c < NC; ++c) rel<T>(x0[ca<K>(c)], x0[cb<K>(c)], G, r0[c]);
    q[0][0] = q[0][1] = q[0][2] = 0;
#pragma unroll
    for (int k = 1; k < NA; ++k) rel<T>(p[0], p[k], G, q[k]);
    int it = 0; bool done = false;
    for (;;) {
        double s[NC][3], sig[3] = {};
        done = true;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int a = ca<K>(c), b = cb<K>(c);
            for (int x = 0; x < 3; ++x) s[c][x] = (q[b][x] + D[b][x]) - (q[a][x] + D[a][x]);
            const double s2 = dot3(s[c], s[c]);
            sig[c] = s2 - dl[c] * dl[c];
            done = done && fabs(sqrt(s2) - dl[c]) <= tol;
        }
        if (done || it >= max_iters) break;
        ++it;
        if constexpr (NC == 1) {
            const double kc = kcoef<K>(0, 0, im), a = kc * kc * dot3(r0[0], r0[0]), b = 2.0 * kc * dot3(s[0], r0[0]), c = sig[0];
            const double disc = b * b - 4.0 * a * c;
            g[0] += (disc >= 0 && b > 0) ? -2.0 * c / (b + sqrt(disc)) : -c / b;      // the root nearer zero; Newton if there is none
        } else {
            double J[3][3] = {}, rhs[3] = {};
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                rhs[c] = -sig[c];
#pragma unroll
                for (int e = 0; e < NC; ++e) J[c][e] = 2.0 * kcoef<K>(c, e, im) * dot3(s[c], r0[e]);
            }
            solve<NC>(J, rhs);
#pragma unroll
            for (int c = 0; c < NC; ++c) g[c] += rhs[c];
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            D[k][0] = D[k][1] = D[k][2] = 0;
#pragma unroll
            for (int e = 0; e < NC; ++e) {
                const double w = (double)((k == cb<K>(e)) - (k == ca<K>(e))) * g[e] * im[k];
                D[k][0] += w * r0[e][0]; D[k][1] += w * r0[e][1]; D[k][2] += w * r0[e][2];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) { p[k].x = (T)((double)p[k].x + D[k][0]); p[k].y = (T)((double)p[k].y + D[k][1]); p[k].z = (T)((double)p[k].z + D[k][2]); }
    return done ? it : -it;
}

// ---- hosted virtual sites (virtual_sites.h): the sites whose parents are all atoms of this item ------------------------------------------
// the position of the item's atom with local number l.  Selected with bit masks: written as a chain of conditional copies the compiler turns the choice
// back into an indexed load, and p[] — with it the whole item — moves from registers to scratch memory.
__device__ inline float mask_if(float v, bool c) { return __uint_as_float(__float_as_uint(v) & (c ? 0xffffffffu : 0u)); }
__device__ inline double mask_if(double v, bool c) { return __longlong_as_double(__double_as_longlong(v) & (c ? -1ll : 0ll)); }
__device__ inline float bits_or(float a, float b) { return __uint_as_float(__float_as_uint(a) | __float_as_uint(b)); }
__device__ inline double bits_or(double a, double b) { return __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(b)); }
template <class T, int NA> __device__ inline typename Vec<T>::T4 pick(const typename Vec<T>::T4* p, int l) {
    typename Vec<T>::T4 r;
    r.x = mask_if(p[0].x, l == 0); r.y = mask_if(p[0].y, l == 0); r.z = mask_if(p[0].z, l == 0); r.w = T(0);
#pragma unroll
    for (int k = 1; k < NA; ++k) { r.x = bits_or(r.x, mask_if(p[k].x, l == k)); r.y = bits_or(r.y, mask_if(p[k].y, l == k)); r.z = bits_or(r.z, mask_if(p[k].z, l == k)); }
    return r;
}
// distribute_forces! for the item's sites: each site's force (of the positions p the forces were computed at) joins its parents' in f[]
template <class T, int NA>
__device__ inline void sites_gather(const ConP<T>& C, const ConStep<T>& A, const GridP<T>& G, int first, int n_vs, const typename Vec<T>::T4* p, typename Vec<T>::T4* f) {
    using T4 = typename Vec<T>::T4;
    for (int j = 0; j < n_vs; ++j) {
        const int32_t* r = C.vs_rec + 4 * (int64_t)(first + j);
        const int type = r[0], l1 = r[2] & 255, l2 = (r[2] >> 8) & 255, l3 = (r[2] >> 16) & 255;
        const int32_t ss = C.inv[r[1]];
        T4 fs = A.frc[ss];
        if (A.fa) { const T4 ga = A.fa[ss]; fs.x += ga.x; fs.y += ga.y; fs.z += ga.z; }
        const T fv[3] = {fs.x, fs.y, fs.z};
        T f1[3], f2[3], f3[3];
        vs_shares<T>(type, pick<T, NA>(p, l1), pick<T, NA>(p, l2), pick<T, NA>(p, l3), C.vs_w + 6 * (int64_t)(first + j), G, fv, f1, f2, f3);
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const bool c1 = k == l1, c2 = type >= VS_TWO_AVG && k == l2, c3 = type >= VS_THREE_AVG && k == l3;      // (masked adds: see pick)
            f[k].x += mask_if(f1[0], c1); f[k].y += mask_if(f1[1], c1); f[k].z += mask_if(f1[2], c1);
            f[k].x += mask_if(f2[0], c2); f[k].y += mask_if(f2[1], c2); f[k].z += mask_if(f2[2], c2);
            f[k].x += mask_if(f3[0], c3); f[k].y += mask_if(f3[1], c3); f[k].z += mask_if(f3[2], c3);
        }
    }
}
// place_virtual_sites! for the item's sites from the wrapped positions p; the sites join the list-validity maxima as the item's atoms do
// (a site with a weight outside [0, 1] or a cross term can move farther than any parent), their speed taken from the move itself
template <class T, int NA>
__device__ inline void sites_place(const ConP<T>& C, const ConStep<T>& A, const GridP<T>& G, int first, int n_vs, const typename Vec<T>::T4* p, T dt, float& da, float& db, float& v2) {
    for (int j = 0; j < n_vs; ++j) {
        const int32_t* r = C.vs_rec + 4 * (int64_t)(first + j);
        const int type = r[0], l1 = r[2] & 255, l2 = (r[2] >> 8) & 255, l3 = (r[2] >> 16) & 255;
        const int32_t ss = C.inv[r[1]];
        auto q = A.pos[ss];
        T x, y, z;
        vs_position<T>(type, pick<T, NA>(p, l1), pick<T, NA>(p, l2), pick<T, NA>(p, l3), C.vs_w + 6 * (int64_t)(first + j), G, x, y, z);
        if (A.trk_part) {
            T ex = x - q.x, ey = y - q.y, ez = z - q.z;
            disp_image(ex, ey, ez, G);
            v2 = fmaxf(v2, (float)((ex * ex + ey * ey + ez * ez) / (dt * dt)));
            auto s = A.snap_a[ss];
            ex = x - s.x; ey = y - s.y; ez = z - s.z;
            disp_image(ex, ey, ez, G);
            da = fmaxf(da, (float)(ex * ex + ey * ey + ez * ez));
            s = A.snap_b[ss];
            ex = x - s.x; ey = y - s.y; ez = z - s.z;
            disp_image(ex, ey, ez, G);
            db = fmaxf(db, (float)(ex * ex + ey * ey + ez * ez));
        }
        q.x = x; q.y = y; q.z = z;
        A.pos[ss] = q;
    }
}

struct Acc { double px = 0, py = 0, pz = 0, m = 0, mv2 = 0; float da = 0.f, db = 0.f, v2 = 0.f; int max_it = 0; int n_fail = 0; };

// one work item: the arithmetic of k_vv1 / k_vv_mid / k_langevin per atom, with RATTLE after every kick and SHAKE after every drift
// TH (a step on which a rescaling thermostat applies, thermostat_step.h): MODE 2 adds Σ m|v|² of the velocities it stores to acc, MODE 0 scales
// v = lam·(v − v_cm) in front of the first kick
template <class T, int K, int MODE, bool TH = false>
__device__ inline void con_item(const ConP<T>& C, const ConStep<T>& A, const GridP<T>& G, int64_t t, const T* vc, bool sub, const T* sh, Acc& acc, T lam = T(1)) {
#pragma clang fp contract(off)
    using T4 = typename Vec<T>::T4;
    constexpr int NA = Shape<K>::NA, NC = Shape<K>::NC;
    if (C.atoms[4 * t] < 0) return;      // padding of a kind's last wave
    int32_t id[NA], sl[NA];
    T4 p[NA], v[NA], f[NA];
    double im[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        id[k] = C.atoms[4 * t + k]; sl[k] = C.inv[id[k]];
        p[k] = A.pos[sl[k]]; v[k] = A.vel[sl[k]]; f[k] = A.frc[sl[k]];
        if (A.fa) { const T4 ga = A.fa[sl[k]]; f[k].x += ga.x; f[k].y += ga.y; f[k].z += ga.z; }
        if constexpr (TH && MODE == 0) thermo_scale<T>(v[k], vc, sub, lam);      // remove_CM_motion! and the thermostat of the step this launch follows
        else if (sub) {                                                        // remove_CM_motion! of the step before, one launch late
            v[k].x -= vc[0]; v[k].y -= vc[1]; v[k].z -= vc[2];
            if constexpr (MODE == 1 || MODE == 2) { p[k].x = M<T>::sub(p[k].x, sh[0]); p[k].y = M<T>::sub(p[k].y, sh[1]); p[k].z = M<T>::sub(p[k].z, sh[2]); }
        }
        im[k] = v[k].w == T(0) ? 0.0 : 1.0 / (double)v[k].w;
    }
    const int vs_first = C.vs_item ? C.vs_item[2 * t] : 0, n_vs = C.vs_item ? C.vs_item[2 * t + 1] : 0;
    if (n_vs > 0) sites_gather<T, NA>(C, A, G, vs_first, n_vs, p, f);                                                // force.jl:796, before the first use of f
    T kx[NA], ky[NA], kz[NA];
    if constexpr (MODE == 1 || MODE == 2) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            kx[k] = M<T>::mul(accel_of(f[k].x, v[k].w), A.dt2); ky[k] = M<T>::mul(accel_of(f[k].y, v[k].w), A.dt2); kz[k] = M<T>::mul(accel_of(f[k].z, v[k].w), A.dt2);
            v[k].x = M<T>::add(v[k].x, kx[k]); v[k].y = M<T>::add(v[k].y, ky[k]); v[k].z = M<T>::add(v[k].z, kz[k]);   // simulators.jl:616
        }
        if constexpr (NC > 0) rattle<T, K>(p, v, im, G);                                                             // :620
        if (A.cm_out)
#pragma unroll
            for (int k = 0; k < NA; ++k) { acc.px += (double)v[k].x * v[k].w; acc.py += (double)v[k].y * v[k].w; acc.pz += (double)v[k].z * v[k].w; acc.m += v[k].w; }
        if constexpr (TH)
#pragma unroll
            for (int k = 0; k < NA; ++k) thermo_accum<T>(v[k], acc.mv2);
    }
    if constexpr (MODE != 2) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if constexpr (MODE == 0) { v[k].x = step_add(v[k].x, accel_of(f[k].x, v[k].w), A.dt2); v[k].y = step_add(v[k].y, accel_of(f[k].y, v[k].w), A.dt2); v[k].z = step_add(v[k].z, accel_of(f[k].z, v[k].w), A.dt2); }
            else if constexpr (MODE == 1) { v[k].x = M<T>::add(v[k].x, kx[k]); v[k].y = M<T>::add(v[k].y, ky[k]); v[k].z = M<T>::add(v[k].z, kz[k]); }   // :594
            else { const T m1 = (v[k].w == T(0)) ? T(0) : T(1) / v[k].w; v[k].x += (f[k].x * m1) * A.S.dt; v[k].y += (f[k].y * m1) * A.S.dt; v[k].z += (f[k].z * m1) * A.S.dt; }   // :1176
        }
        if constexpr (NC > 0) rattle<T, K>(p, v, im, G);                                                             // :596 / :1180
        T4 x0[NA], pu[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            x0[k] = p[k];
            if constexpr (MODE != 3) { p[k].x = step_add(p[k].x, v[k].x, A.dt); p[k].y = step_add(p[k].y, v[k].y, A.dt); p[k].z = step_add(p[k].z, v[k].z, A.dt); }   // :602
            else {                                                             // :1187-1192, kernels.jl:739
                const StochP<T>& P = A.S;
                p[k].x = fma_t(P.dt_half, v[k].x, p[k].x); p[k].y = fma_t(P.dt_half, v[k].y, p[k].y); p[k].z = fma_t(P.dt_half, v[k].z, p[k].z);
                T z[3];
                randn3<T>((uint64_t)id[k] + 1, P.ctr1, P.key, P.natoms, z);
                const T ns = thermal_scale<T>(P.noise_kt, v[k].w);
                v[k].x = fma_t(P.vel_scale, v[k].x, z[0] * ns); v[k].y = fma_t(P.vel_scale, v[k].y, z[1] * ns); v[k].z = fma_t(P.vel_scale, v[k].z, z[2] * ns);
                p[k].x = fma_t(P.dt_half, v[k].x, p[k].x); p[k].y = fma_t(P.dt_half, v[k].y, p[k].y); p[k].z = fma_t(P.dt_half, v[k].z, p[k].z);
            }
            pu[k] = p[k];
        }
        if constexpr (NC > 0) {
            const double dl[3] = {C.d[4 * t], C.d[4 * t + 1], C.d[4 * t + 2]};
            const int it = shake<T, K>(x0, p, im, dl, C.tol, C.max_iters, G);                                         // :605 / :1195
            acc.max_it = max(acc.max_it, it < 0 ? -it : it);
            acc.n_fail += it < 0;
            const T dt = MODE == 3 ? A.S.dt : A.dt;
#pragma unroll
            for (int k = 0; k < NA; ++k) {                                     // v += (x_constrained − x_unconstrained)/dt
                v[k].x += (p[k].x - pu[k].x) / dt; v[k].y += (p[k].y - pu[k].y) / dt; v[k].z += (p[k].z - pu[k].z) / dt;
            }
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) wrap_point(p[k].x, p[k].y, p[k].z, G);                                          // :609 / :1201
        if constexpr (MODE == 3)
            if (A.cm_out)
#pragma unroll
                for (int k = 0; k < NA; ++k) { acc.px += (double)v[k].x * v[k].w; acc.py += (double)v[k].y * v[k].w; acc.pz += (double)v[k].z * v[k].w; acc.m += v[k].w; }
    }
    if (n_vs > 0 && (MODE != 2 || sub)) sites_place<T, NA>(C, A, G, vs_first, n_vs, p, MODE == 3 ? A.S.dt : A.dt, acc.da, acc.db, acc.v2);   // :610 / :1187, wherever the parents moved
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (MODE != 2 || sub) A.pos[sl[k]] = p[k];
        A.vel[sl[k]] = v[k];
        if (A.trk_part) {
            acc.v2 = fmaxf(acc.v2, (float)(v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z));
            auto q = A.snap_a[sl[k]];
            T ex = p[k].x - q.x, ey = p[k].y - q.y, ez = p[k].z - q.z;
            disp_image(ex, ey, ez, G);
            acc.da = fmaxf(acc.da, (float)(ex * ex + ey * ey + ez * ez));
            q = A.snap_b[sl[k]];
            ex = p[k].x - q.x; ey = p[k].y - q.y; ez = p[k].z - q.z;
            disp_image(ex, ey, ez, G);
            acc.db = fmaxf(acc.db, (float)(ex * ex + ey * ey + ez * ez));
        }
    }
}

template <class T, int MODE, bool TH>
__device__ __forceinline__ void con_step_body(const ConP<T>& C, const ConStep<T>& A, const GridP<T>& G, const ThermoArgs& X) {
    static_assert(!TH || MODE == 0 || MODE == 2, "the thermostat's launches: close (2) and open (0)");
    T vc[3] = {T(0), T(0), T(0)};
    [[maybe_unused]] T lam = T(1);
    const bool sub = A.vcm != nullptr || A.cm_in != nullptr;
    if constexpr (TH && MODE == 0) lam = thermo_block_lambda<T>(A.cm_in, X.th_in, A.n_cm_in, X.th, vc);      // (the open launch: cm_in, th_in are the close launch's partials)
    else if (A.cm_in) block_vcm<T>(A.cm_in, A.n_cm_in, vc);
    else if (A.vcm) { vc[0] = A.vcm[0]; vc[1] = A.vcm[1]; vc[2] = A.vcm[2]; }
    const T sh[3] = {M<T>::mul(vc[0], A.dt), M<T>::mul(vc[1], A.dt), M<T>::mul(vc[2], A.dt)};
    Acc acc;
    const int64_t n = C.end[CK_N - 1], stride = (int64_t)gridDim.x * blockDim.x;      // (a multiple of the wave: a wave stays within one kind)
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += stride) {
        if (t < C.end[CK_2]) con_item<T, CK_2, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else if (t < C.end[CK_3]) con_item<T, CK_3, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else if (t < C.end[CK_4]) con_item<T, CK_4, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else if (t < C.end[CK_ANGLE]) con_item<T, CK_ANGLE, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else if (t < C.end[CK_FREE]) con_item<T, CK_FREE, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else if (t < C.end[CK_G2]) con_item<T, CK_G2, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else if (t < C.end[CK_G3]) con_item<T, CK_G3, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
        else con_item<T, CK_G4, MODE, TH>(C, A, G, t, vc, sub, sh, acc, lam);
    }
    // the solver's counters: one vector atomic per wave into device words the host reads with the run's other read-backs
    int mi = acc.max_it;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mi = max(mi, __shfl_xor(mi, o, 64));
    int nf = acc.n_fail;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if ((threadIdx.x & 63) == 0 && C.stat) {
        if (mi > 0) atomicMax(&C.stat[1], (unsigned long long)mi);
        if (nf > 0) atomicAdd(&C.stat[0], (unsigned long long)nf);
    }
    if (A.trk_part) block_trk_write(acc.da, acc.db, acc.v2, A.trk_part);
    if (A.cm_out) block_cm_write(acc.px, acc.py, acc.pz, acc.m, A.cm_out);
    if constexpr (TH && MODE == 2) thermo_write_partial(acc.mv2, thermo_noise_share<T>(X.th), X.th_out);
}

template <class T, int MODE>
__global__ void __launch_bounds__(CON_BLOCK) k_con_step(ConP<T> C, ConStep<T> A, GridP<T> G) { con_step_body<T, MODE, false>(C, A, G, ThermoArgs{}); }
// the close (MODE 2) and open (MODE 0) launches of a step on which a rescaling thermostat applies (thermostat_step.h)
template <class T, int MODE>
__global__ void __launch_bounds__(CON_BLOCK) k_con_thermo(ConP<T> C, ConStep<T> A, GridP<T> G, ThermoArgs X) { con_step_body<T, MODE, true>(C, A, G, X); }

}  // namespace

template <class T>
void launch_con_step(hipStream_t s, int nb, int mode, const ConP<T>& C, const ConStep<T>& A, const GridP<T>& G, const ThermoArgs* X) {
    if (X) {      // a coupled step's close (2) and open (0)
        if (mode == 2) hipLaunchKernelGGL((k_con_thermo<T, 2>), dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G, *X);
        else hipLaunchKernelGGL((k_con_thermo<T, 0>), dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G, *X);
        return;
    }
    switch (mode) {
    case 0: hipLaunchKernelGGL((k_con_step<T, 0>), dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G); break;
    case 1: hipLaunchKernelGGL((k_con_step<T, 1>), dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G); break;
    case 2: hipLaunchKernelGGL((k_con_step<T, 2>), dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G); break;
    default: hipLaunchKernelGGL((k_con_step<T, 3>), dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G); break;
    }
}
template void launch_con_step<float>(hipStream_t, int, int, const ConP<float>&, const ConStep<float>&, const GridP<float>&, const ThermoArgs*);
template void launch_con_step<double>(hipStream_t, int, int, const ConP<double>&, const ConStep<double>&, const GridP<double>&, const ThermoArgs*);

// ---- the constraint virial of the state held (mhip_constraint_virial; merge_initial_constraint_virial!, simulators.jl:459-495) ------------
namespace {

// The trial step is carried in double, relative to the cluster's first atom: x[k] is the minimum-image vector first atom → atom k of the UNMOVED
// coordinates (shake.jl:239-243's local_coord), and the virial is accumulated from the solvers' own corrections dv[] and D[] — never from a
// difference of values rounded to T (a SHAKE correction of the preview step is some 1e-5 nm, an fp32 ulp at 3 nm 2.4e-7 nm).

// RATTLE as rattle() above, on bond vectors r and velocities v in double: dv[k] is the correction of atom k, v is left as it was
template <int K> __device__ inline void vir_rattle(const double (*r)[3], const double (*v)[3], const double* im, double (*dv)[3]) {
    constexpr int NA = Shape<K>::NA, NC = Shape<K>::NC;
    double A[3][3] = {}, b[3] = {};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double u[3] = {v[cb<K>(c)][0] - v[ca<K>(c)][0], v[cb<K>(c)][1] - v[ca<K>(c)][1], v[cb<K>(c)][2] - v[ca<K>(c)][2]};
        b[c] = -dot3(r[c], u);
#pragma unroll
        for (int e = 0; e < NC; ++e) A[c][e] = kcoef<K>(c, e, im) * dot3(r[c], r[e]);
    }
    solve<NC>(A, b);
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        dv[k][0] = dv[k][1] = dv[k][2] = 0;
#pragma unroll
        for (int e = 0; e < NC; ++e) {
            const double w = (double)((k == cb<K>(e)) - (k == ca<K>(e))) * b[e] * im[k];
            dv[k][0] += w * r[e][0]; dv[k][1] += w * r[e][1]; dv[k][2] += w * r[e][2];
        }
    }
}

// SHAKE as shake() above, on drifted positions q relative to the first atom: D[k] is the correction of atom k along the bonds r0 of the unmoved
// coordinates.  Returns the iterations taken, negative when max_iters ran out first.
template <int K> __device__ inline int vir_shake(const double (*r0)[3], const double (*q)[3], const double* im, const double* dl, double tol, int max_iters, double (*D)[3]) {
    constexpr int NA = Shape<K>::NA, NC = Shape<K>::NC;
    double g[NC] = {};
#pragma unroll
    for (int k = 0; k < NA; ++k) D[k][0] = D[k][1] = D[k][2] = 0;
    int it = 0; bool done = false;
    for (;;) {
        double s[NC][3], sig[3] = {};
        done = true;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int a = ca<K>(c), b = cb<K>(c);
#pragma unroll
            for (int x = 0; x < 3; ++x) s[c][x] = (q[b][x] + D[b][x]) - (q[a][x] + D[a][x]);
            const double s2 = dot3(s[c], s[c]);
            sig[c] = s2 - dl[c] * dl[c];
            done = done && fabs(sqrt(s2) - dl[c]) <= tol;
        }
        if (done || it >= max_iters) break;
        ++it;
        if constexpr (NC == 1) {
            const double kc = kcoef<K>(0, 0, im), a = kc * kc * dot3(r0[0], r0[0]), b = 2.0 * kc * dot3(s[0], r0[0]), c = sig[0];
            const double disc = b * b - 4.0 * a * c;
            g[0] += (disc >= 0 && b > 0) ? -2.0 * c / (b + sqrt(disc)) : -c / b;      // the root nearer zero; Newton if there is none
        } else {
            double J[3][3] = {}, rhs[3] = {};
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                rhs[c] = -sig[c];
#pragma unroll
                for (int e = 0; e < NC; ++e) J[c][e] = 2.0 * kcoef<K>(c, e, im) * dot3(s[c], r0[e]);
            }
            solve<NC>(J, rhs);
#pragma unroll
            for (int c = 0; c < NC; ++c) g[c] += rhs[c];
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            D[k][0] = D[k][1] = D[k][2] = 0;
#pragma unroll
            for (int e = 0; e < NC; ++e) {
                const double w = (double)((k == cb<K>(e)) - (k == ca<K>(e))) * g[e] * im[k];
                D[k][0] += w * r0[e][0]; D[k][1] += w * r0[e][1]; D[k][2] += w * r0[e][2];
            }
        }
    }
    return done ? it : -it;
}

// W[0..8] += λ_c/dt · Σ_k x_k ⊗ m_k dv_k (RATTLE of the kicked velocities), W[9..17] += λ_c/dt² · Σ_k x_k ⊗ m_k D_k (SHAKE of the drifted positions);
// row-major, W[3a + b] = x_a · impulse_b (shake.jl:244-246)
template <class T, int K>
__device__ inline void con_virial_item(const ConP<T>& C, const ConVirial<T>& A, const GridP<T>& G, int64_t t, double* W, int& n_fail) {
    constexpr int NA = Shape<K>::NA, NC = Shape<K>::NC;
    if (C.atoms[4 * t] < 0) return;      // padding of a kind's last wave
    double x[NA][3], v[NA][3], kick[NA][3], m[NA], im[NA], lam = 1.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int32_t id = C.atoms[4 * t + k], sl = C.inv[id];
        const auto p = A.pos[sl], u = A.vel[sl];
        m[k] = (double)u.w; im[k] = u.w == T(0) ? 0.0 : 1.0 / (double)u.w;
        x[k][0] = p.x; x[k][1] = p.y; x[k][2] = p.z;
        v[k][0] = u.x; v[k][1] = u.y; v[k][2] = u.z;
#pragma unroll
        for (int c = 0; c < 3; ++c) kick[k][c] = u.w == T(0) ? 0.0 : (double)A.f[3 * (int64_t)id + c] / m[k] * A.dt;      // accels .* dt (:482)
        if (A.lam) lam = fmin(lam, (double)A.lam[id]);                                                                    // MinimumMixing (constraints.jl:94-117)
    }
#pragma unroll
    for (int k = NA - 1; k >= 0; --k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double d = x[k][c] - x[0][c];
            if (G.periodic[c]) d -= (double)G.L[c] * rint(d / (double)G.L[c]);
            x[k][c] = d;
        }
    double r[NC][3], dv[NA][3];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) r[c][a] = x[cb<K>(c)][a] - x[ca<K>(c)][a];
    vir_rattle<K>(r, v, im, dv);                                                                                          // :479, accumulates nothing
#pragma unroll
    for (int k = 0; k < NA; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] += dv[k][c] + kick[k][c];                                                     // :482
    vir_rattle<K>(r, v, im, dv);                                                                                          // :484
    const double sv = lam / A.dt, sp = lam / (A.dt * A.dt);
#pragma unroll
    for (int k = 1; k < NA; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) W[3 * a + b] += sv * x[k][a] * (m[k] * dv[k][b]);
    double q[NA][3], D[NA][3];
#pragma unroll
    for (int k = 0; k < NA; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] += dv[k][c];
#pragma unroll
    for (int k = 0; k < NA; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) q[k][c] = x[k][c] + (v[k][c] - v[0][c]) * A.dt;                                       // :486, relative to the first atom
    const double dl[3] = {C.d[4 * t], C.d[4 * t + 1], C.d[4 * t + 2]};
    const int it = vir_shake<K>(r, q, im, dl, C.tol, C.max_iters, D);                                                     // :488
    n_fail += it < 0;
#pragma unroll
    for (int k = 1; k < NA; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) W[9 + 3 * a + b] += sp * x[k][a] * (m[k] * D[k][b]);
}

// one lane per cluster of the kinds CK_2 … CK_ANGLE (a wave stays within one kind), a grid-stride loop, one wave per block; reads pos, vel, λ and the
// caller's forces, writes nothing but part[c · gridDim.x + block], c < 18 the components of Wv then Wp, c = 18 the solves that stopped at max_iters
template <class T>
__global__ void __launch_bounds__(CON_BLOCK) k_con_virial(ConP<T> C, ConVirial<T> A, GridP<T> G) {
    double W[18] = {};
    int nf = 0;
    const int64_t n = C.end[CK_ANGLE], stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += stride) {
        if (t < C.end[CK_2]) con_virial_item<T, CK_2>(C, A, G, t, W, nf);
        else if (t < C.end[CK_3]) con_virial_item<T, CK_3>(C, A, G, t, W, nf);
        else if (t < C.end[CK_4]) con_virial_item<T, CK_4>(C, A, G, t, W, nf);
        else con_virial_item<T, CK_ANGLE>(C, A, G, t, W, nf);
    }
#pragma unroll
    for (int c = 0; c < 18; ++c) {
        double w = W[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
        if (threadIdx.x == 0) A.part[(size_t)c * gridDim.x + blockIdx.x] = w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if (threadIdx.x == 0) A.part[(size_t)18 * gridDim.x + blockIdx.x] = (double)nf;
}

}  // namespace

template <class T>
void launch_con_virial(hipStream_t s, int nb, const ConP<T>& C, const ConVirial<T>& A, const GridP<T>& G) {
    hipLaunchKernelGGL(k_con_virial<T>, dim3(nb), dim3(CON_BLOCK), 0, s, C, A, G);
}
template void launch_con_virial<float>(hipStream_t, int, const ConP<float>&, const ConVirial<float>&, const GridP<float>&);
template void launch_con_virial<double>(hipStream_t, int, const ConP<double>&, const ConVirial<double>&, const GridP<double>&);

}  // namespace mhip
