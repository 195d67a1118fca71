// virtual_sites.h — virtual sites (src/virtual.jl): massless atoms whose position is a function of up to three parent atoms and whose
// force belongs to those parents.
//
// Two forms.  The one-shot kernels k_vs_place / k_vs_spread (virtual_sites.hip, one lane per site) serve mhip_place_virtual_sites,
// mhip_distribute_forces and the start of a run.  Inside the step loops a site is HOSTED by the work item of k_con_step that owns
// all of its parents (constraints.h): the lane gathers the site's force into the parents' registers before the kick and writes the
// site's position behind the wrap — no launch of its own, no atomics.  Both forms call the two functions below, so a site placed by
// either is the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "physics.h"

namespace mhip {

enum { VS_ONE = 1, VS_TWO_AVG = 2, VS_THREE_AVG = 3, VS_OUT_OF_PLANE = 4 };   // virtual.jl:11

// the sites as the caller gave them: 0-based caller indices (−1: unused parent), w = (weight_1, weight_2, weight_3, weight_12,
// weight_13, weight_cross) per site
struct SiteSet {
    std::vector<int32_t> type, site, a1, a2, a3;
    std::vector<double> w;
    std::vector<uint8_t> flag;         // per atom: is a site
    int64_t n = 0;
    int64_t n_type[4] = {0, 0, 0, 0};
};
// throws ApiError{MHIP_ERR_INVALID} as setup_virtual_sites does (virtual.jl:120-180): a type outside 1..4, an index out of range, an atom
// defined twice, a parent that is a site, weights of an average that do not sum to one
SiteSet build_sites(int64_t n_atoms, int64_t n, const int32_t* type, const int32_t* site, const int32_t* a1, const int32_t* a2, const int32_t* a3,
                    const double* w6);

// one record per site for the one-shot kernels: rec[8s ..] = (type, site, a1, a2, a3, ·, ·, ·), w[6s ..]
template <class T> struct VsP {
    int64_t n;
    const int32_t* rec; const double* w; const int32_t* inv;
};

template <class T>
void launch_vs_place(hipStream_t s, const VsP<T>& V, typename Vec<T>::T4* pos, const GridP<T>& G, int32_t* changed);
// f: the caller's packed xyz array in caller order; pos (through inv) gives r12, r13 of an out-of-plane site
template <class T>
void launch_vs_spread(hipStream_t s, const VsP<T>& V, const typename Vec<T>::T4* pos, T* f, const GridP<T>& G);

// nearest-image vector a → b and the wrap, as min_image_exact / wrap_point compute them in an orthorhombic box — their triclinic branch is left out
// (sites with a TriclinicBoundary are refused), so every use inlines and the out-values stay in registers
template <class T> __device__ inline void vs_image(const typename Vec<T>::T4& a, const typename Vec<T>::T4& b, const GridP<T>& G, T* d) {
    d[0] = G.periodic[0] ? vector_1d_exact(a.x, b.x, G.L[0]) : M<T>::sub(b.x, a.x);
    d[1] = G.periodic[1] ? vector_1d_exact(a.y, b.y, G.L[1]) : M<T>::sub(b.y, a.y);
    d[2] = G.periodic[2] ? vector_1d_exact(a.z, b.z, G.L[2]) : M<T>::sub(b.z, a.z);
}
template <class T> __device__ inline void vs_wrap(T& x, T& y, T& z, const GridP<T>& G) {
    if (G.periodic[0]) x = wrap_1d(x, G.L[0]);
    if (G.periodic[1]) y = wrap_1d(y, G.L[1]);
    if (G.periodic[2]) z = wrap_1d(z, G.L[2]);
}

// ---- device: the arithmetic both forms share (every operation individually rounded, so that both give the same bits) -----------------------
// position of a site from its parents' (virtual.jl:198-222): only r1 is absolute, the others enter as nearest-image vectors from it
template <class T>
__device__ inline void vs_position(int type, const typename Vec<T>::T4& p1, const typename Vec<T>::T4& p2, const typename Vec<T>::T4& p3,
                                   const double* w, const GridP<T>& G, T& x, T& y, T& z) {
#pragma clang fp contract(off)
    x = p1.x; y = p1.y; z = p1.z;
    if (type >= VS_TWO_AVG) {
        T a[3], b[3] = {T(0), T(0), T(0)};
        vs_image<T>(p1, p2, G, a);
        if (type >= VS_THREE_AVG) vs_image<T>(p1, p3, G, b);
        const T wa = (T)(type == VS_OUT_OF_PLANE ? w[3] : w[1]), wb = (T)(type == VS_OUT_OF_PLANE ? w[4] : w[2]);
        x = x + wa * a[0]; y = y + wa * a[1]; z = z + wa * a[2];
        if (type >= VS_THREE_AVG) { x = x + wb * b[0]; y = y + wb * b[1]; z = z + wb * b[2]; }
        if (type == VS_OUT_OF_PLANE) {
            const T wc = (T)w[5];
            x = x + wc * (a[1] * b[2] - a[2] * b[1]); y = y + wc * (a[2] * b[0] - a[0] * b[2]); z = z + wc * (a[0] * b[1] - a[1] * b[0]);
        }
    }
    vs_wrap(x, y, z, G);
}

// the parents' shares of a site's force f (virtual.jl:247-287): the transposed Jacobian of vs_position.  With r = r1 + a r12 + b r13 +
// c (r12 × r13): F2 = a f + c (r13 × f), F3 = b f + c (f × r12), F1 = f − F2 − F3.
template <class T>
__device__ inline void vs_shares(int type, const typename Vec<T>::T4& p1, const typename Vec<T>::T4& p2, const typename Vec<T>::T4& p3,
                                 const double* w, const GridP<T>& G, const T* f, T* f1, T* f2, T* f3) {
#pragma clang fp contract(off)
    // (scalars throughout, one straight path: arrays written on two paths end up in scratch memory)
    const bool oop = type == VS_OUT_OF_PLANE;
    T a[3] = {T(0), T(0), T(0)}, b[3] = {T(0), T(0), T(0)};
    if (oop) { vs_image<T>(p1, p2, G, a); vs_image<T>(p1, p3, G, b); }
    const T wa = (T)(oop ? w[3] : (type >= VS_TWO_AVG ? w[1] : 0.0)), wb = (T)(oop ? w[4] : (type == VS_THREE_AVG ? w[2] : 0.0)), wc = (T)(oop ? w[5] : 0.0);
    const T fx = f[0], fy = f[1], fz = f[2];
    const T g2x = wa * fx + wc * (b[1] * fz - b[2] * fy), g2y = wa * fy + wc * (b[2] * fx - b[0] * fz), g2z = wa * fz + wc * (b[0] * fy - b[1] * fx);
    const T g3x = wb * fx + wc * (fy * a[2] - fz * a[1]), g3y = wb * fy + wc * (fz * a[0] - fx * a[2]), g3z = wb * fz + wc * (fx * a[1] - fy * a[0]);
    // the first parent takes the rest: f − F2 − F3 for an out-of-plane site, w1 f for an average (w1 = 1 for a one-particle site)
    const T w1 = type == VS_ONE ? T(1) : (T)w[0];
    f1[0] = oop ? fx - g2x - g3x : w1 * fx; f1[1] = oop ? fy - g2y - g3y : w1 * fy; f1[2] = oop ? fz - g2z - g3z : w1 * fz;
    f2[0] = g2x; f2[1] = g2y; f2[2] = g2z;
    f3[0] = g3x; f3[1] = g3y; f3[2] = g3z;
}

}  // namespace mhip
