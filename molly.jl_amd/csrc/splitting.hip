// splitting.hip — LangevinSplitting (simulators.jl:1212-1398) and OverdampedLangevin (:1400-1489) on the device: one launch runs a whole segment of
// A / B / O sub-steps (splitting.h) on an atom in registers (see split_kernel.h)
#include "split_kernel.h"

#include "integrate.h"
#include "philox.h"

namespace mhip {

namespace {

// Per atom, the sub-steps of the segment in order, every operation individually rounded (an explicit fma only where the reference's kernel has one):
//   A  x += v·h, then wrap                                                                A_step!, :1383-1388
//   B  v += h·(F·(1/m)), the kick of langevin_atom; forces as the pass in front left them B_step!, :1390-1398
//   O  v = fma(vel_scale_i, v, noise_scale_i·ξ), a_i = o_rate / m_i, vel_scale_i = exp(−a_i), noise_scale_i = sqrt(kT/m_i·(1 − exp(−2 a_i))): both in
//      double from the atom's mass, rounded once to T (the convention of thermal_scale); ξ = randn3(orig + 1, the sub-step's ctr1, key)   :1282-1289, kernels.jl:726-741
//   overdamped  x += ((F/m)/γ)·h + sqrt(2h/γ)·(sqrt(kT/m)·ξ), then wrap                    :1464-1466
// An atom of mass 0 (a virtual site: M_inv = 0, :1272-1275) is left alone by B, O and the overdamped update; A still moves it.
// In front the deferred remove_CM_motion! of the step before, behind (CM) the Σ m v partials of this one.  Only what changed is stored.
template <class T, bool CM>
__global__ void __launch_bounds__(256) k_split_segment(int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* __restrict__ frc,
                                                       const int32_t* __restrict__ orig, SplitProg<T> P, const T* __restrict__ vcm, const double* __restrict__ cm_in,
                                                       int n_cm_in, double* cm_out, GridP<T> G) {
#pragma clang fp contract(off)
    T vc[3];
    const bool sub = pending_vcm<T>(vcm, cm_in, n_cm_in, vc);
    const bool reads_frc = P.kicks || P.op[0] == SPLIT_OVERDAMPED;
    double px = 0, py = 0, pz = 0, m = 0;
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto v = vel[s]; auto p = pos[s];
        auto f = make4<T>(T(0), T(0), T(0), T(0));
        if (reads_frc) f = frc[s];
        if (sub) cm_remove(v, vc);
        const bool massless = v.w == T(0);
        const T im = massless ? T(0) : T(1) / v.w;                             // calc_accels, force.jl:17
        T vel_scale = T(1), noise_scale = T(0);
        if (P.noise && !massless) {
            const double a = P.o_rate / (double)v.w;
            vel_scale = (T)::exp(-a);
            noise_scale = (T)::sqrt(P.kT / (double)v.w * (1.0 - ::exp(-2.0 * a)));
        }
        const uint64_t ctr0 = (uint64_t)orig[s] + 1;
        for (int j = 0; j < P.n; ++j) {                                        // (uniform across the wave: the program is in the kernel arguments)
            const int32_t op = P.op[j];
            const T h = P.dt[j];
            if (op == SPLIT_A) {
                p.x += v.x * h; p.y += v.y * h; p.z += v.z * h;
                wrap_point(p.x, p.y, p.z, G);
            } else if (op == SPLIT_B) {
                v.x += h * (f.x * im); v.y += h * (f.y * im); v.z += h * (f.z * im);
            } else if (op == SPLIT_O) {
                if (!massless) {
                    T z[3];
                    randn3<T>(ctr0, P.ctr1[j], P.key, P.natoms, z);
                    v.x = fma_t(vel_scale, v.x, noise_scale * z[0]); v.y = fma_t(vel_scale, v.y, noise_scale * z[1]); v.z = fma_t(vel_scale, v.z, noise_scale * z[2]);
                }
            } else if (!massless) {
                T z[3];
                randn3<T>(ctr0, P.ctr1[j], P.key, P.natoms, z);
                const T sc = thermal_scale<T>(P.kT, v.w);
                p.x += ((f.x * im) / P.od_gamma) * h + P.od_prefac * (z[0] * sc);
                p.y += ((f.y * im) / P.od_gamma) * h + P.od_prefac * (z[1] * sc);
                p.z += ((f.z * im) / P.od_gamma) * h + P.od_prefac * (z[2] * sc);
                wrap_point(p.x, p.y, p.z, G);
            }
        }
        if (P.kicks || P.noise || sub) vel[s] = v;
        if (P.moves) pos[s] = p;
        if constexpr (CM) { px += (double)v.x * v.w; py += (double)v.y * v.w; pz += (double)v.z * v.w; m += v.w; }
    }
    if constexpr (CM) block_cm_write(px, py, pz, m, cm_out);
}

}  // namespace

template <class T>
void launch_split_segment(hipStream_t s, int n_blocks, int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* frc,
                          const int32_t* orig, const SplitProg<T>& P, const T* vcm, const double* cm_in, int n_cm_in, double* cm_out, const GridP<T>& G) {
    if (cm_out) hipLaunchKernelGGL((k_split_segment<T, true>), dim3(n_blocks), dim3(256), 0, s, n, pos, vel, frc, orig, P, vcm, cm_in, n_cm_in, cm_out, G);
    else hipLaunchKernelGGL((k_split_segment<T, false>), dim3(n_blocks), dim3(256), 0, s, n, pos, vel, frc, orig, P, vcm, cm_in, n_cm_in, cm_out, G);
}

template void launch_split_segment<float>(hipStream_t, int, int64_t, float4*, float4*, const float4*, const int32_t*, const SplitProg<float>&, const float*, const double*, int, double*, const GridP<float>&);
template void launch_split_segment<double>(hipStream_t, int, int64_t, double4*, double4*, const double4*, const int32_t*, const SplitProg<double>&, const double*, const double*, int, double*, const GridP<double>&);

}  // namespace mhip
