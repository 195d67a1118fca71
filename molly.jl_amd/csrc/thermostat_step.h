// thermostat_step.h — the device side of the rescaling thermostats (thermostat.h) in the velocity-Verlet step loop.
// On a step where the thermostat applies, the integrator stage is two launches instead of one:
//   close  closing kick (+ RATTLE), the Σ m v partials as always, and per block one THERMOSTAT PARTIAL {Σ m|v|², Σ ξ²} (thermo_accum /
//          thermo_noise_share / thermo_write_partial, called by k_vv_close and k_con_thermo<…, 2>);
//   open   every block re-sums both partial arrays in the same fixed order (thermo_block_lambda), calls thermostat_lambda, scales
//          v = λ·(v − v_cm) and carries on with the first kick, the drift and the wrap (k_vv_open, k_con_thermo<…, 0>).
// The run's last step has no open: k_scale_vel applies the same λ·(v − v_cm) in the same operation order.  (The helpers are here, the
// kernels with the integrators they belong to: integrate.h, constraints.hip.)
// CSVR noise: atom i (caller index) owns the three normals randn3(i + 1, ctr1 + step, key) — the ones mhip_random_velocities would draw
// for it; numbered k = 3i + c, R is k = 0 and S = Σ ξ_k² over 1 <= k <= dof − 1.  The close launch's lanes stride over the CALLER
// indices, so the sum depends neither on the sorted order of the moment nor on how a run is cut into calls.
#pragma once
#include "philox.h"
#include "physics.h"
#include "thermostat.h"

namespace mhip {

// ---- close ---------------------------------------------------------------------------------------------------------------------------
template <class T, class T4> __device__ inline void thermo_accum(const T4& v, double& mv2) {
    mv2 += (double)v.w * ((double)v.x * (double)v.x + (double)v.y * (double)v.y + (double)v.z * (double)v.z);
}
// this lane's share of S: the normals 1 <= k <= dof − 1 of the caller indices it strides over
template <class T> __device__ inline double thermo_noise_share(const ThermoP& P) {
    double xi2 = 0;
    if (P.kind != THERMO_CSVR || P.dof < 2) return xi2;
    const int64_t k_last = P.dof - 1, n_i = min((int64_t)P.natoms, k_last / 3 + 1);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_i; i += (int64_t)gridDim.x * blockDim.x) {
        T z[3];
        randn3<T>((uint64_t)i + 1, P.ctr1, P.key, P.natoms, z);
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int64_t k = 3 * i + c; if (k >= 1 && k <= k_last) xi2 += (double)z[c] * (double)z[c]; }
    }
    return xi2;
}
// th_out[2·block + {0, 1}] = the block's {Σ m|v|², Σ ξ²}: waves by shuffle, then the waves in order (block_cm_write's order, integrate.h)
__device__ inline void thermo_write_partial(double mv2, double xi2, double* th_out) {
    __shared__ double sh_th[16][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mv2 += __shfl_xor(mv2, o, 64); xi2 += __shfl_xor(xi2, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh_th[threadIdx.x >> 6][0] = mv2; sh_th[threadIdx.x >> 6][1] = xi2; }
    __syncthreads();
    if (threadIdx.x < 2) { double a = 0; for (int q = 0; q < (int)(blockDim.x >> 6); ++q) a += sh_th[q][threadIdx.x]; th_out[2 * (int64_t)blockIdx.x + threadIdx.x] = a; }
}

// ---- open ----------------------------------------------------------------------------------------------------------------------------
// Every block: the n_part partials of the close launch re-summed in block_cm_total's order (cm_part null: the step removes no CM motion),
// v_cm = P / M rounded to T as block_vcm does, λ in double rounded to T once.  Block 0 keeps the info record.
// (Six values wide, one barrier: sharing block_cm_total's four would mean a second re-sum for the thermostat's two, with its own barrier, or a branch
// on the caller inside the shared one — it stays a sum of its own, in the same order.  blockDim.x <= 1024.)
template <class T>
__device__ inline T thermo_block_lambda(const double* __restrict__ cm_part, const double* __restrict__ th_part, int n_part, const ThermoP& P, T* vcm3) {
    __shared__ double sh_tl[16][6];
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int q = threadIdx.x; q < n_part; q += blockDim.x) {
        if (cm_part) { const double* p = cm_part + 4 * (int64_t)q; a[0] += p[0]; a[1] += p[1]; a[2] += p[2]; a[3] += p[3]; }
        a[4] += th_part[2 * (int64_t)q]; a[5] += th_part[2 * (int64_t)q + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) for (int c = 0; c < 6; ++c) a[c] += __shfl_xor(a[c], o, 64);
    if ((threadIdx.x & 63) == 0) for (int c = 0; c < 6; ++c) sh_tl[threadIdx.x >> 6][c] = a[c];
    __syncthreads();
    double t[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) for (int c = 0; c < 6; ++c) t[c] += sh_tl[q][c];
    const bool cm = cm_part != nullptr;
    for (int c = 0; c < 3; ++c) vcm3[c] = cm ? (T)(t[c] / t[3]) : T(0);
    double R = 0;
    if (P.kind == THERMO_CSVR) { T z[3]; randn3<T>(1, P.ctr1, P.key, P.natoms, z); R = (double)z[0]; }
    double K = 0; int32_t refused = 0;
    const double lam = thermostat_lambda(P.kind, t[4], t, t[3], cm, P.dof, P.kT, P.dt, P.tau, P.n_steps, R, t[5], &K, &refused);
    if (blockIdx.x == 0 && threadIdx.x == 0 && P.info) {
        double* o = P.info;
        const bool first = o[0] == 0.0;
        o[0] += 1.0; o[1] = (double)P.step; o[2] = lam; o[3] = K;
        o[4] = first ? lam : fmin(o[4], lam); o[5] = first ? lam : fmax(o[5], lam);
        o[6] += (double)refused;
    }
    return (T)lam;
}
// v = λ·(v − v_cm): the subtraction first, each operation rounded in T
template <class T, class T4> __device__ inline void thermo_scale(T4& v, const T* vc, bool sub, T lam) {
    if (sub) { v.x = M<T>::sub(v.x, vc[0]); v.y = M<T>::sub(v.y, vc[1]); v.z = M<T>::sub(v.z, vc[2]); }
    v.x = M<T>::mul(lam, v.x); v.y = M<T>::mul(lam, v.y); v.z = M<T>::mul(lam, v.z);
}

}  // namespace mhip
