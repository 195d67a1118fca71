// minimize.h — the device side of mhip_minimize: simulate!(sys, ::SteepestDescentMinimizer) (simulators.jl:183-271) on the coordinates the context holds.
//
// The engine's loop (engine.hip, minimize) launches, per step: the total force of the step (step_forces, the side array folded in), the harmonic bonds that
// stand in for the constraints (k_min_cbonds), the sites' forces onto their parents (k_min_spread), max ‖F‖ (k_min_maxf), the move (k_min_move: keeps the old
// coordinates, x += (hn·F)/max_force, wrap), the sites' placement, the three energy passes with their sums left in device words (k_min_sum), the decision
// (k_min_decide), the restore of a rejected step with the displacement of the coordinates that stand against the lists' snapshots (k_min_settle) and the copy
// of the record into pinned host words (k_min_publish).  The host waits for that record once per step and reads nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.h"
#include "constraints.h"
#include "virtual_sites.h"

namespace mhip {

constexpr int MIN_MAX_BLOCKS = 1024;      // per-block partials of the reductions, as the other reductions of the engine

// the record of a minimisation, doubles, on the device and (copied by k_min_publish) in pinned host words
enum {
    MR_E = 0,         // the potential energy of the coordinates that stand
    MR_HN,            // the step length of the next move, carried in the context's precision
    MR_E_TRIAL,       // the last step's trial energy
    MR_MAXF,          // … its max ‖F‖
    MR_ACCEPTED,      // … 1 / 0
    MR_HN_USED,       // … the step length it moved by
    MR_STEPS, MR_N_ACC, MR_N_REJ,
    MR_E0,            // the energy before the first step
    MR_DISP_IN2,      // max |x − snapshot|² of the coordinates that stand: against the inner (or only) list's snapshot | the outer list's
    MR_DISP_OUT2,
    MR_N
};
// the device words the energy passes' sums go to
enum { MS_PAIR = 0, MS_SPEC, MS_GEN, MS_CBOND, MS_N };

// which parts the total has, added in the order pair, specific (+ constraint bonds), general; gen = 0.5·Σ + gen_const (ewald.jl:917-928)
struct MinParts { int pair, spec, gen, cbond; double gen_const; };

// the constraint clusters as k_min_cbonds reads them: the items [0, end[CK_ANGLE]) of the engine's ClusterSet
template <class T> struct MinBonds {
    const int32_t* atoms; const double* d; const int32_t* inv;
    int32_t end[4];      // CK_2, CK_3, CK_4, CK_ANGLE
    T k;
};

// out[slot] = Σ part[0 .. n) in the fixed order of the engine's k_sum_double
void launch_min_sum(hipStream_t s, int n, const double* part, double* out);
// max ‖F‖² per block of the owned slots → part[0 .. n_blocks); returns n_blocks <= MIN_MAX_BLOCKS
template <class T> int launch_min_maxf(hipStream_t s, int64_t n, const typename Vec<T>::T4* frc, T* part);
// keep[orig[s]] = pos[s];  pos[s] += (hn·F)/max_force, wrapped (nothing moves when max_force == 0);  rec[MR_MAXF], rec[MR_HN_USED]
template <class T>
void launch_min_move(hipStream_t s, int64_t n, typename Vec<T>::T4* pos, const typename Vec<T>::T4* frc, const int32_t* orig, typename Vec<T>::T4* keep, const T* part, int n_part,
                     double* rec, const GridP<T>& G);
// the harmonic bonds k/2·(r − d)² of the constrained pairs: forces ADDED to frc (energy == false), or one energy partial per block → part (returns the block count)
template <class T>
int launch_min_cbonds(hipStream_t s, const MinBonds<T>& B, const typename Vec<T>::T4* pos, typename Vec<T>::T4* frc, double* part, bool energy, const GridP<T>& G);
// distribute_forces! on the engine's own force array (slot order): every site's row onto its parents' rows, then zeroed
template <class T>
void launch_min_spread(hipStream_t s, const VsP<T>& V, const typename Vec<T>::T4* pos, typename Vec<T>::T4* frc, const GridP<T>& G);
// init: E = E0 = the total, hn = step_size, counters zero;  else the step's decision: E_trial < E → E = E_trial, hn = 6·hn/5; otherwise hn = hn/5
template <class T> void launch_min_decide(hipStream_t s, double* rec, const double* sums, const MinParts& P, bool init, double step_size);
// restore: a rejected step (rec[MR_ACCEPTED] == 0) takes its coordinates back from keep.  Either way the displacement of the coordinates that stand against
// snap_in / snap_out (nullable) goes to dpart (two floats per block); returns the block count
template <class T>
int launch_min_settle(hipStream_t s, int64_t n, typename Vec<T>::T4* pos, const int32_t* orig, const typename Vec<T>::T4* keep, const double* rec, bool restore,
                      const typename Vec<T>::T4* snap_in, const typename Vec<T>::T4* snap_out, float* dpart, const GridP<T>& G);
// the step's last launch: the displacement maxima into the record, the record into the pinned words
void launch_min_publish(hipStream_t s, int n_part, const float* dpart, double* rec, double* host_rec);

}  // namespace mhip
