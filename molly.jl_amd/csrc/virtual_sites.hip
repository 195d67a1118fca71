// virtual_sites.hip — the site set's validation and the one-shot placement / force-spreading kernels (see virtual_sites.h)
#include "virtual_sites.h"

#include <cmath>
#include <limits>

namespace mhip {

// ---- host: setup_virtual_sites (virtual.jl:120-152) and the constructors' weight checks (:70-73, :92-95) -----------------------------
SiteSet build_sites(int64_t n_atoms, int64_t n, const int32_t* type, const int32_t* site, const int32_t* a1, const int32_t* a2, const int32_t* a3,
                    const double* w6) {
    auto bad = [](const std::string& m) { return ApiError{MHIP_ERR_INVALID, "virtual sites: " + m}; };
    if (n < 0) throw bad("negative count");
    if (!type || !site || !a1 || !a2 || !a3 || !w6) throw bad("null array");
    auto in_range = [&](int32_t a) { return a >= 0 && (int64_t)a < n_atoms; };
    // isapprox(x, 1) with the default tolerances: |x − 1| <= √eps · max(|x|, 1)
    auto is_one = [](double x) { return std::fabs(x - 1.0) <= std::sqrt(std::numeric_limits<double>::epsilon()) * std::max(std::fabs(x), 1.0); };
    SiteSet s;
    s.n = n; s.flag.assign((size_t)n_atoms, 0);
    for (int64_t k = 0; k < n; ++k) {
        const std::string where = "site " + std::to_string(k);
        if (type[k] < VS_ONE || type[k] > VS_OUT_OF_PLANE) throw bad(where + " has type " + std::to_string(type[k]) + " (1..4)");
        if (!in_range(site[k])) throw bad(where + " defines an atom out of range");
        if (s.flag[site[k]]) throw bad(where + " defines atom " + std::to_string(site[k]) + ", which an earlier site already defines");
        s.flag[site[k]] = 1;
        const int np = type[k] == VS_ONE ? 1 : (type[k] == VS_TWO_AVG ? 2 : 3);
        const int32_t par[3] = {a1[k], a2[k], a3[k]};
        for (int m = 0; m < np; ++m)
            if (!in_range(par[m])) throw bad(where + " has a parent out of range");
        const double* w = w6 + 6 * k;
        for (int m = 0; m < 6; ++m)
            if (!std::isfinite(w[m])) throw bad(where + " has a weight that is not finite");
        if (type[k] == VS_TWO_AVG && !is_one(w[0] + w[1])) throw bad(where + ": weight_1 + weight_2 must equal 1");
        if (type[k] == VS_THREE_AVG && !is_one(w[0] + w[1] + w[2])) throw bad(where + ": weight_1 + weight_2 + weight_3 must equal 1");
        s.type.push_back(type[k]); s.site.push_back(site[k]);
        s.a1.push_back(par[0]); s.a2.push_back(np > 1 ? par[1] : -1); s.a3.push_back(np > 2 ? par[2] : -1);
        s.w.insert(s.w.end(), w, w + 6);
        ++s.n_type[type[k] - 1];
    }
    for (int64_t k = 0; k < n; ++k)
        for (int32_t p : {s.a1[k], s.a2[k], s.a3[k]})
            if (p >= 0 && s.flag[p]) throw bad("site " + std::to_string(k) + " is defined in terms of atom " + std::to_string(p) + ", which is itself a site");
    return s;
}

// ---- device --------------------------------------------------------------------------------------------------------------------------
namespace {

template <class T>
__global__ void __launch_bounds__(256) k_vs_place(VsP<T> V, typename Vec<T>::T4* pos, GridP<T> G, int32_t* changed) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= V.n) return;
    const int32_t* r = V.rec + 8 * s;
    const int type = r[0];
    const auto p1 = pos[V.inv[r[2]]];
    auto p2 = p1, p3 = p1;
    if (type >= VS_TWO_AVG) p2 = pos[V.inv[r[3]]];
    if (type >= VS_THREE_AVG) p3 = pos[V.inv[r[4]]];
    const int32_t slot = V.inv[r[1]];
    auto q = pos[slot];
    T x, y, z;
    vs_position<T>(type, p1, p2, p3, V.w + 6 * s, G, x, y, z);
    if (changed && (x != q.x || y != q.y || z != q.z)) *changed = 1;      // (a site that already sits where its parents put it leaves the state as it was)
    q.x = x; q.y = y; q.z = z;
    pos[slot] = q;
}

template <class T>
__global__ void __launch_bounds__(256) k_vs_spread(VsP<T> V, const typename Vec<T>::T4* __restrict__ pos, T* f, GridP<T> G) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= V.n) return;
    const int32_t* r = V.rec + 8 * s;
    const int type = r[0];
    typename Vec<T>::T4 p1{}, p2{}, p3{};
    if (type == VS_OUT_OF_PLANE) { p1 = pos[V.inv[r[2]]]; p2 = pos[V.inv[r[3]]]; p3 = pos[V.inv[r[4]]]; }
    T* fs = f + 3 * (int64_t)r[1];
    const T fv[3] = {fs[0], fs[1], fs[2]};
    T f1[3], f2[3], f3[3];
    vs_shares<T>(type, p1, p2, p3, V.w + 6 * s, G, fv, f1, f2, f3);
    // several sites may share a parent: hardware float atomics (one global_atomic_add per component)
    T* g1 = f + 3 * (int64_t)r[2];
    unsafeAtomicAdd(g1, f1[0]); unsafeAtomicAdd(g1 + 1, f1[1]); unsafeAtomicAdd(g1 + 2, f1[2]);
    if (type >= VS_TWO_AVG) { T* g2 = f + 3 * (int64_t)r[3]; unsafeAtomicAdd(g2, f2[0]); unsafeAtomicAdd(g2 + 1, f2[1]); unsafeAtomicAdd(g2 + 2, f2[2]); }
    if (type >= VS_THREE_AVG) { T* g3 = f + 3 * (int64_t)r[4]; unsafeAtomicAdd(g3, f3[0]); unsafeAtomicAdd(g3 + 1, f3[1]); unsafeAtomicAdd(g3 + 2, f3[2]); }
    fs[0] = T(0); fs[1] = T(0); fs[2] = T(0);                             // virtual.jl:290-292
}

}  // namespace

template <class T>
void launch_vs_place(hipStream_t s, const VsP<T>& V, typename Vec<T>::T4* pos, const GridP<T>& G, int32_t* changed) {
    if (V.n <= 0) return;
    hipLaunchKernelGGL(k_vs_place<T>, dim3(cdiv(V.n, 256)), dim3(256), 0, s, V, pos, G, changed);
}
template <class T>
void launch_vs_spread(hipStream_t s, const VsP<T>& V, const typename Vec<T>::T4* pos, T* f, const GridP<T>& G) {
    if (V.n <= 0) return;
    hipLaunchKernelGGL(k_vs_spread<T>, dim3(cdiv(V.n, 256)), dim3(256), 0, s, V, pos, f, G);
}
template void launch_vs_place<float>(hipStream_t, const VsP<float>&, float4*, const GridP<float>&, int32_t*);
template void launch_vs_place<double>(hipStream_t, const VsP<double>&, double4*, const GridP<double>&, int32_t*);
template void launch_vs_spread<float>(hipStream_t, const VsP<float>&, const float4*, float*, const GridP<float>&);
template void launch_vs_spread<double>(hipStream_t, const VsP<double>&, const double4*, double*, const GridP<double>&);

}  // namespace mhip
