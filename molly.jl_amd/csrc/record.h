// record.h — the recorder's kernels: what apply_loggers! (loggers.jl:44-56) reads of a step's state, taken on the device so that a run need not be cut.
//   k_record        one pass over the owned atoms in their current sorted order: the pending Σ m v removal (flush_cm's effect, k_shift_vel's arithmetic),
//                   the block's kinetic-energy partial (k_ke_partials' arithmetic and reduction order) and the rows of the coordinate and velocity
//                   frames in caller order (what k_gather_state hands out), each only when asked for
//   k_record_recip  the PME energy 0.5·Σ partials + constant in k_sum_double's order, as pme_energy() finishes it on the host
// The sums of the other channels are folded into their slots by k_sum_double itself (integrate.h).
#pragma once
#include "integrate.h"

namespace mhip {

// One 256-lane block per 256 atoms.  vcm / cm_part, n_cm_part: the pending removal as PendingCm hands it to a launch (both null: none); skip (nullable):
// per caller index, atoms whose velocity is left alone (virtual sites, spatial.jl:926).  ke_part (nullable): one partial per block.  frame_x / frame_v
// (nullable): 3·n values each, packed xyz, row orig[s] — a scatter: the pass runs in sorted order because the kinetic-energy partials are defined in
// it and the velocities are read (and written back) there anyway; the 12-byte rows of one wave land within the few cache lines of its cell's neighbours
// after a sort by cell and anywhere in the frame when the caller's order is unrelated to space.
template <class T>
__global__ void __launch_bounds__(256) k_record(int64_t n, const typename Vec<T>::T4* __restrict__ pos, typename Vec<T>::T4* vel, const T* __restrict__ vcm,
                                                const double* __restrict__ cm_part, int n_cm_part, const int32_t* __restrict__ orig, const uint8_t* __restrict__ skip,
                                                double* ke_part, T* frame_x, T* frame_v) {
    T vc[3];
    const bool sub = pending_vcm<T>(vcm, cm_part, n_cm_part, vc);
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double k = 0;
    if (s < n) {
        auto v = vel[s];
        const int64_t o = orig[s];
        if (sub && !(skip && skip[o])) { cm_remove(v, vc); vel[s] = v; }
        k = ke_atom(v);
        if (frame_v) { frame_v[3 * o] = v.x; frame_v[3 * o + 1] = v.y; frame_v[3 * o + 2] = v.z; }
        if (frame_x) { const auto p = pos[s]; frame_x[3 * o] = p.x; frame_x[3 * o + 1] = p.y; frame_x[3 * o + 2] = p.z; }
    }
    if (!ke_part) return;      // (uniform over the grid)
    __shared__ double sh[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) { double a = 0; for (int q = 0; q < (int)(blockDim.x >> 6); ++q) a += sh[q]; ke_part[blockIdx.x] = a; }
}

// out[0] = 0.5·Σ part[0 .. n) + add, the sum in k_sum_double's order (ewald.jl:917-928).  One block of 256 lanes.
[[maybe_unused]] static __global__ void k_record_recip(int n, const double* __restrict__ part, double add, double* out) {
    __shared__ double sh[256];
    double a = 0;
    for (int q = threadIdx.x; q < n; q += blockDim.x) a += part[q];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int q = 0; q < (int)blockDim.x; ++q) t += sh[q]; out[0] = __dadd_rn(__dmul_rn(0.5, t), add); }
}

}  // namespace mhip
