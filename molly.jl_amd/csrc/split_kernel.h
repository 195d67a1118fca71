// split_kernel.h — the launch of one segment of a LangevinSplitting step, or of one OverdampedLangevin update (splitting.hip; the plan: splitting.h)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.h"
#include "splitting.h"

namespace mhip {

// the program of one launch, by value in the kernel arguments: at most SPLIT_MAX_OPS sub-steps, run per atom in registers
template <class T> struct SplitProg {
    int32_t n = 0;
    int32_t op[SPLIT_MAX_OPS];        // SplitOp
    T dt[SPLIT_MAX_OPS];              // the effective time step of the sub-step
    uint64_t ctr1[SPLIT_MAX_OPS];     // an O, the overdamped update: the Philox counter of this sub-step
    bool moves = false, kicks = false, noise = false;      // the segment has an A (or the overdamped update) | a B | an O
    double o_rate = 0;                // O: friction·dt / n_O, so that a_i = o_rate / m_i                        simulators.jl:1282
    double kT = 0;                    // O: kT; overdamped: sqrt(kT), the scale of random_velocities!            :1283, :1464
    T od_gamma = T(1), od_prefac = T(0);      // overdamped: γ, sqrt((2/γ)·dt)                                    :1454
    uint64_t key = 0, natoms = 0;
};

// one launch over the owned atoms (blocks of 256 lanes, grid stride); vcm / cm_in: the pending centre-of-mass removal, applied in front;
// cm_out (nullable): 4 doubles per block (Σ m v, Σ m) of the velocities the launch leaves
template <class T>
void launch_split_segment(hipStream_t s, int n_blocks, int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* frc,
                          const int32_t* orig, const SplitProg<T>& P, const T* vcm, const double* cm_in, int n_cm_in, double* cm_out, const GridP<T>& G);

}  // namespace mhip
