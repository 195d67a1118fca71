// minimize.hip — the kernels of mhip_minimize (see minimize.h): the decisions of the steepest-descent loop taken on the device, so that forces, trial
// coordinates and energies never cross to the host.  gfx950, wave64; templated on the context's precision.
#include "minimize.h"

#include <algorithm>

#include "bonded.h"
#include "kernels.h"

namespace mhip {
namespace {

constexpr int MIN_BLOCK = 256;

// the larger of the two, a NaN winning over every number (maximum(norm.(F)) of the reference propagates it)
template <class T> __device__ inline T nan_max(T a, T b) { return (b > a || b != b) ? b : a; }
template <class T> __device__ inline T wave_nan_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, (T)__shfl_xor(v, o, 64));
    return v;
}
// the block's maximum, returned to every lane (256 lanes = 4 waves)
template <class T> __device__ inline T block_nan_max(T v) {
    __shared__ T sh[MIN_BLOCK / WAVE];
    v = wave_nan_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T m = sh[0];
#pragma unroll
    for (int q = 1; q < MIN_BLOCK / WAVE; ++q) m = nan_max(m, sh[q]);
    __syncthreads();
    return m;
}

__global__ void __launch_bounds__(256) k_min_sum(int n, const double* __restrict__ part, double* out) {
    __shared__ double sh[256];
    double a = 0;
    for (int q = threadIdx.x; q < n; q += blockDim.x) a += part[q];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int q = 0; q < (int)blockDim.x; ++q) t += sh[q]; out[0] = t; }
}

template <class T>
__global__ void __launch_bounds__(MIN_BLOCK) k_min_maxf(int64_t n, const typename Vec<T>::T4* __restrict__ frc, T* part) {
#pragma clang fp contract(off)
    T m = T(0);
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const auto f = frc[s];
        m = nan_max(m, (f.x * f.x + f.y * f.y) + f.z * f.z);
    }
    m = block_nan_max(m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

template <class T>
__global__ void __launch_bounds__(MIN_BLOCK) k_min_move(int64_t n, typename Vec<T>::T4* pos, const typename Vec<T>::T4* __restrict__ frc, const int32_t* __restrict__ orig,
                                                        typename Vec<T>::T4* keep, const T* __restrict__ part, int n_part, double* rec, GridP<T> G) {
#pragma clang fp contract(off)
    // every block reduces the partials itself: a maximum is exact in any order, so all blocks agree
    T m = T(0);
    for (int q = threadIdx.x; q < n_part; q += blockDim.x) m = nan_max(m, part[q]);
    const T max_force = M<T>::sqrt(block_nan_max(m));
    const T hn = (T)rec[MR_HN];
    const bool still = max_force == T(0);      // nothing to move along: the loop stops as converged, without the division
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto p = pos[s];
        keep[orig[s]] = p;
        if (still) continue;
        const auto f = frc[s];
        p.x = p.x + (hn * f.x) / max_force; p.y = p.y + (hn * f.y) / max_force; p.z = p.z + (hn * f.z) / max_force;
        wrap_point(p.x, p.y, p.z, G);
        pos[s] = p;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec[MR_MAXF] = (double)max_force; rec[MR_HN_USED] = (double)hn; }
}

// one pair of a cluster: the harmonic bond of bonded.h (d_bonds) with the constraint's length
template <class T, bool ENERGY>
__device__ inline void cbond(const typename Vec<T>::T4& pa, const typename Vec<T>::T4& pb, T k, T r0, const GridP<T>& G, T* fa, T* fb, double& e) {
    T ab[3];
    min_image_exact<T>(pa.x, pa.y, pa.z, pb.x, pb.y, pb.z, G, ab[0], ab[1], ab[2]);
    const T r = M<T>::sqrt(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]);
    const T dr = r - r0;
    if constexpr (ENERGY) e += (double)((k / T(2)) * dr * dr);
    else {
        const T c = k * dr / r;
#pragma unroll
        for (int a = 0; a < 3; ++a) { fa[a] += c * ab[a]; fb[a] -= c * ab[a]; }
    }
}

// one lane per constraint cluster.  An atom is in at most one cluster, so the lane owns its atoms' force rows: plain loads and stores.
template <class T, bool ENERGY>
__global__ void __launch_bounds__(MIN_BLOCK) k_min_cbonds(MinBonds<T> B, const typename Vec<T>::T4* __restrict__ pos, typename Vec<T>::T4* frc, double* part, GridP<T> G) {
    const int n_items = B.end[3];
    double e = 0;
    for (int t = blockIdx.x * (int)blockDim.x + threadIdx.x; t < n_items; t += (int)(gridDim.x * blockDim.x)) {
        const int32_t* a = B.atoms + 4 * (int64_t)t;
        if (a[0] < 0) continue;      // padding of a kind's range
        const int kind = t < B.end[0] ? 0 : (t < B.end[1] ? 1 : (t < B.end[2] ? 2 : 3));
        const int na = kind == 3 ? 3 : kind + 2;
        int slot[4] = {0, 0, 0, 0};
        typename Vec<T>::T4 p[4];
        T f[4][3] = {{T(0), T(0), T(0)}, {T(0), T(0), T(0)}, {T(0), T(0), T(0)}, {T(0), T(0), T(0)}};
#pragma unroll
        for (int m = 0; m < 4; ++m) if (m < na) { slot[m] = B.inv[a[m]]; p[m] = pos[slot[m]]; }
        const double* d = B.d + 4 * (int64_t)t;
        if (kind == 3) {      // (i, j = centre, k) with d = (d_ij, d_jk, d_ik): all three sides
            cbond<T, ENERGY>(p[0], p[1], B.k, (T)d[0], G, f[0], f[1], e);
            cbond<T, ENERGY>(p[1], p[2], B.k, (T)d[1], G, f[1], f[2], e);
            cbond<T, ENERGY>(p[0], p[2], B.k, (T)d[2], G, f[0], f[2], e);
        } else {              // the centre first, then its 1, 2 or 3 satellites
            cbond<T, ENERGY>(p[0], p[1], B.k, (T)d[0], G, f[0], f[1], e);
            if (kind >= 1) cbond<T, ENERGY>(p[0], p[2], B.k, (T)d[1], G, f[0], f[2], e);
            if (kind >= 2) cbond<T, ENERGY>(p[0], p[3], B.k, (T)d[2], G, f[0], f[3], e);
        }
        if constexpr (!ENERGY) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < na) { auto g = frc[slot[m]]; g.x += f[m][0]; g.y += f[m][1]; g.z += f[m][2]; frc[slot[m]] = g; }
        }
    }
    if constexpr (ENERGY) block_sum_to(e, part);
}

// k_vs_spread of virtual_sites.hip on the engine's own force array: rows addressed through inv[]
template <class T>
__global__ void __launch_bounds__(256) k_min_spread(VsP<T> V, const typename Vec<T>::T4* __restrict__ pos, typename Vec<T>::T4* frc, GridP<T> G) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= V.n) return;
    const int32_t* r = V.rec + 8 * s;
    const int type = r[0];
    const int s0 = V.inv[r[1]], s1 = V.inv[r[2]];
    const int s2 = type >= VS_TWO_AVG ? V.inv[r[3]] : s1, s3 = type >= VS_THREE_AVG ? V.inv[r[4]] : s1;
    typename Vec<T>::T4 p1{}, p2{}, p3{};
    if (type == VS_OUT_OF_PLANE) { p1 = pos[s1]; p2 = pos[s2]; p3 = pos[s3]; }
    auto fs = frc[s0];
    const T fv[3] = {fs.x, fs.y, fs.z};
    T f1[3], f2[3], f3[3];
    vs_shares<T>(type, p1, p2, p3, V.w + 6 * s, G, fv, f1, f2, f3);
    // several sites may share a parent: hardware float atomics, as the caller-order form
    unsafeAtomicAdd(&frc[s1].x, f1[0]); unsafeAtomicAdd(&frc[s1].y, f1[1]); unsafeAtomicAdd(&frc[s1].z, f1[2]);
    if (type >= VS_TWO_AVG) { unsafeAtomicAdd(&frc[s2].x, f2[0]); unsafeAtomicAdd(&frc[s2].y, f2[1]); unsafeAtomicAdd(&frc[s2].z, f2[2]); }
    if (type >= VS_THREE_AVG) { unsafeAtomicAdd(&frc[s3].x, f3[0]); unsafeAtomicAdd(&frc[s3].y, f3[1]); unsafeAtomicAdd(&frc[s3].z, f3[2]); }
    fs.x = T(0); fs.y = T(0); fs.z = T(0);                                 // virtual.jl:290-292
    frc[s0] = fs;
}

template <class T>
__global__ void k_min_decide(double* rec, const double* __restrict__ sums, MinParts P, int init, double step_size) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double e = 0.0;      // the parts in the order potential_energy adds them
    if (P.pair) e += sums[MS_PAIR];
    if (P.spec || P.cbond) e += (P.spec ? sums[MS_SPEC] : 0.0) + (P.cbond ? sums[MS_CBOND] : 0.0);
    if (P.gen) e += 0.5 * sums[MS_GEN] + P.gen_const;
    if (init) {
        for (int k = 0; k < MR_N; ++k) rec[k] = 0.0;
        rec[MR_E] = e; rec[MR_E0] = e; rec[MR_HN] = (double)(T)step_size;
        rec[MR_ACCEPTED] = 1.0;      // (nothing to take back)
        return;
    }
    T hn = (T)rec[MR_HN];
    const bool accepted = e < rec[MR_E];      // a NaN energy rejects
    if (accepted) { hn = T(6) * hn / T(5); rec[MR_E] = e; rec[MR_N_ACC] += 1.0; }
    else { hn = hn / T(5); rec[MR_N_REJ] += 1.0; }
    rec[MR_HN] = (double)hn; rec[MR_E_TRIAL] = e; rec[MR_ACCEPTED] = accepted ? 1.0 : 0.0; rec[MR_STEPS] += 1.0;
}

template <class T>
__global__ void __launch_bounds__(MIN_BLOCK) k_min_settle(int64_t n, typename Vec<T>::T4* pos, const int32_t* __restrict__ orig, const typename Vec<T>::T4* __restrict__ keep,
                                                          const double* __restrict__ rec, int restore, const typename Vec<T>::T4* __restrict__ snap_in,
                                                          const typename Vec<T>::T4* __restrict__ snap_out, float* dpart, GridP<T> G) {
    const bool back = restore && rec[MR_ACCEPTED] == 0.0;
    float da = 0.f, db = 0.f;
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto p = pos[s];
        if (back) { const auto q = keep[orig[s]]; p.x = q.x; p.y = q.y; p.z = q.z; pos[s] = p; }
        if (snap_in) da = nan_max(da, disp2_from(p.x, p.y, p.z, snap_in[s], G));
        if (snap_out) db = nan_max(db, disp2_from(p.x, p.y, p.z, snap_out[s], G));
    }
    da = block_nan_max(da);
    db = block_nan_max(db);
    if (threadIdx.x == 0) { dpart[2 * blockIdx.x] = da; dpart[2 * blockIdx.x + 1] = db; }
}

__global__ void __launch_bounds__(MIN_BLOCK) k_min_publish(int n_part, const float* __restrict__ dpart, double* rec, double* host_rec) {
    float da = 0.f, db = 0.f;
    for (int q = threadIdx.x; q < n_part; q += blockDim.x) { da = nan_max(da, dpart[2 * q]); db = nan_max(db, dpart[2 * q + 1]); }
    da = block_nan_max(da);
    db = block_nan_max(db);
    if (threadIdx.x == 0) {
        rec[MR_DISP_IN2] = (double)da; rec[MR_DISP_OUT2] = (double)db;
        for (int k = 0; k < MR_N; ++k) host_rec[k] = rec[k];
    }
}

int grid_of(int64_t n) { return std::max(1, std::min(cdiv(n, MIN_BLOCK), MIN_MAX_BLOCKS)); }

}  // namespace

void launch_min_sum(hipStream_t s, int n, const double* part, double* out) { hipLaunchKernelGGL(k_min_sum, dim3(1), dim3(256), 0, s, n, part, out); }

template <class T> int launch_min_maxf(hipStream_t s, int64_t n, const typename Vec<T>::T4* frc, T* part) {
    const int nb = grid_of(n);
    hipLaunchKernelGGL(k_min_maxf<T>, dim3(nb), dim3(MIN_BLOCK), 0, s, n, frc, part);
    return nb;
}
template <class T>
void launch_min_move(hipStream_t s, int64_t n, typename Vec<T>::T4* pos, const typename Vec<T>::T4* frc, const int32_t* orig, typename Vec<T>::T4* keep, const T* part, int n_part,
                     double* rec, const GridP<T>& G) {
    hipLaunchKernelGGL(k_min_move<T>, dim3(grid_of(n)), dim3(MIN_BLOCK), 0, s, n, pos, frc, orig, keep, part, n_part, rec, G);
}
template <class T>
int launch_min_cbonds(hipStream_t s, const MinBonds<T>& B, const typename Vec<T>::T4* pos, typename Vec<T>::T4* frc, double* part, bool energy, const GridP<T>& G) {
    const int nb = grid_of(B.end[3]);
    if (energy) hipLaunchKernelGGL((k_min_cbonds<T, true>), dim3(nb), dim3(MIN_BLOCK), 0, s, B, pos, frc, part, G);
    else hipLaunchKernelGGL((k_min_cbonds<T, false>), dim3(nb), dim3(MIN_BLOCK), 0, s, B, pos, frc, part, G);
    return nb;
}
template <class T>
void launch_min_spread(hipStream_t s, const VsP<T>& V, const typename Vec<T>::T4* pos, typename Vec<T>::T4* frc, const GridP<T>& G) {
    if (V.n <= 0) return;
    hipLaunchKernelGGL(k_min_spread<T>, dim3(cdiv(V.n, 256)), dim3(256), 0, s, V, pos, frc, G);
}
template <class T> void launch_min_decide(hipStream_t s, double* rec, const double* sums, const MinParts& P, bool init, double step_size) {
    hipLaunchKernelGGL(k_min_decide<T>, dim3(1), dim3(64), 0, s, rec, sums, P, init ? 1 : 0, step_size);
}
template <class T>
int launch_min_settle(hipStream_t s, int64_t n, typename Vec<T>::T4* pos, const int32_t* orig, const typename Vec<T>::T4* keep, const double* rec, bool restore,
                      const typename Vec<T>::T4* snap_in, const typename Vec<T>::T4* snap_out, float* dpart, const GridP<T>& G) {
    const int nb = grid_of(n);
    hipLaunchKernelGGL(k_min_settle<T>, dim3(nb), dim3(MIN_BLOCK), 0, s, n, pos, orig, keep, rec, restore ? 1 : 0, snap_in, snap_out, dpart, G);
    return nb;
}
void launch_min_publish(hipStream_t s, int n_part, const float* dpart, double* rec, double* host_rec) {
    hipLaunchKernelGGL(k_min_publish, dim3(1), dim3(MIN_BLOCK), 0, s, n_part, dpart, rec, host_rec);
}

#define MHIP_MIN_INST(T, T4)                                                                                                                                              \
    template int launch_min_maxf<T>(hipStream_t, int64_t, const T4*, T*);                                                                                                 \
    template void launch_min_move<T>(hipStream_t, int64_t, T4*, const T4*, const int32_t*, T4*, const T*, int, double*, const GridP<T>&);                                 \
    template int launch_min_cbonds<T>(hipStream_t, const MinBonds<T>&, const T4*, T4*, double*, bool, const GridP<T>&);                                                   \
    template void launch_min_spread<T>(hipStream_t, const VsP<T>&, const T4*, T4*, const GridP<T>&);                                                                      \
    template void launch_min_decide<T>(hipStream_t, double*, const double*, const MinParts&, bool, double);                                                               \
    template int launch_min_settle<T>(hipStream_t, int64_t, T4*, const int32_t*, const T4*, const double*, bool, const T4*, const T4*, float*, const GridP<T>&);
MHIP_MIN_INST(float, float4)
MHIP_MIN_INST(double, double4)
#undef MHIP_MIN_INST

}  // namespace mhip
