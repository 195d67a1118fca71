// integrate.h — the integrator stage of the step: the stand-alone velocity-Verlet kernels and the block-level pieces that every integrator
// kernel shares (these, k_langevin / k_redraw of stochastic.hip, the constrained steps of constraints.hip).
// The bit-for-bit guarantees of the step loops — a run continued in chunks repeats the uncut run, the fused step repeats the separate
// integrator, the thermostat's flush equals its open launch — hold because every kernel performs the same operations in the same association
// and sums waves in the same order.  That contract is the code below and the per-atom pieces in kernels.h (lone_kick / drift,
// cm_remove, disp2_from, cm_partials_wave_sum).  Three bodies write the same operations out, because through the helpers the compiler gave them
// more registers or another instruction stream: the STEP epilogue of k_forces (its stream is held fixed; nothing k_forces calls lives here),
// vv_mid_body below (per-atom pieces and its Σ m v write) and con_item / con_step_body's prologue in constraints.hip.
//   cm_out[4·block + c]            the block's {Σ m vx, Σ m vy, Σ m vz, Σ m}       block_cm_write → block_vcm / pending_vcm
//   trk_part[c·gridDim.x + block]  the block's largest |x − snap_a|², |x − snap_b|², |v|²: the validity check of the pair lists, taken
//                                  where the new coordinates are made                block_trk_write
// Each helper owns its static LDS; none is called twice in one kernel.
#pragma once
#include "kernels.h"
#include "thermostat_step.h"

namespace mhip {

// The block's Σ m v partial: waves by butterfly, then the waves in order.  blockDim.x <= 256 (sh[4] waves).
__device__ inline void block_cm_write(double px, double py, double pz, double m, double* cm_out) {
    __shared__ double sh[4][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { px += __shfl_xor(px, o, 64); py += __shfl_xor(py, o, 64); pz += __shfl_xor(pz, o, 64); m += __shfl_xor(m, o, 64); }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[w][0] = px; sh[w][1] = py; sh[w][2] = pz; sh[w][3] = m; }
    __syncthreads();
    if (threadIdx.x < 4) { double a = 0; for (int q = 0; q < (int)(blockDim.x >> 6); ++q) a += sh[q][threadIdx.x]; cm_out[4 * (int64_t)blockIdx.x + threadIdx.x] = a; }
}
// The block's three maxima of the list check.  blockDim.x <= 1024 (sht[16] waves).
__device__ inline void block_trk_write(float da, float db, float v2, float* trk_part) {
    __shared__ float sht[3][16];
    da = wave_max(da); db = wave_max(db); v2 = wave_max(v2);
    if ((threadIdx.x & 63) == 0) { sht[0][threadIdx.x >> 6] = da; sht[1][threadIdx.x >> 6] = db; sht[2][threadIdx.x >> 6] = v2; }
    __syncthreads();
    if (threadIdx.x < 3) { float m = 0.f; for (int q = 0; q < (int)(blockDim.x >> 6); ++q) m = fmaxf(m, sht[threadIdx.x][q]); trk_part[threadIdx.x * gridDim.x + blockIdx.x] = m; }
}
// v_cm = Σ(m v) / Σ m of n_part partials, in EVERY lane and in one fixed order (cm_partials_wave_sum of kernels.h, then the waves in order), rounded to T
// once: any number of blocks re-sum the same partials to the same bits (n_part <= 1024, 32 KB of L2 reads per block), so no finalize launch has to
// sit between the kernel that wrote them and the one that needs v_cm.  k_cm_finalize and k_halo_pack's head block end the same sum in one lane.
// blockDim.x <= 256.
template <class T>
__device__ inline void block_vcm(const double* __restrict__ part, int n_part, T* vcm3) {
    __shared__ double sh_cm[4][4];
    double a[4];
    cm_partials_wave_sum(part, n_part, a);
    if ((threadIdx.x & 63) == 0) for (int c = 0; c < 4; ++c) sh_cm[threadIdx.x >> 6][c] = a[c];
    __syncthreads();
    double t[4] = {0, 0, 0, 0};
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) for (int c = 0; c < 4; ++c) t[c] += sh_cm[q][c];
    for (int c = 0; c < 3; ++c) vcm3[c] = (T)(t[c] / t[3]);
}
// The removal a launch finds pending: v_cm from the partials of the launch before (cm_part), or as a finished vector (vcm), or none (zeros).
// Returns whether there is one.  blockDim.x <= 256.
template <class T>
__device__ inline bool pending_vcm(const T* __restrict__ vcm, const double* __restrict__ cm_part, int n_part, T* vc) {
    vc[0] = vc[1] = vc[2] = T(0);
    if (cm_part) block_vcm<T>(cm_part, n_part, vc);
    else if (vcm) { vc[0] = vcm[0]; vc[1] = vcm[1]; vc[2] = vcm[2]; }
    return vcm != nullptr || cm_part != nullptr;
}

// ---------------------------------------------------------------------------------------------------
// velocity Verlet (simulators.jl:589-629), owned atoms, sorted order.  vel.w carries the mass.
// The integrator's arithmetic is the reference's, operation by operation (no fused multiply-add, a true division): a = f / m with 0 for
// massless atoms (calc_accels, force.jl:17), v += a·dt/2 (simulators.jl:594, 616), x += v·dt (:602).  Every kernel below goes through
// the per-atom pieces of kernels.h, so a run cut into chunks repeats the uncut run bit for bit (test/simulation.jl:16-57).

template <class T>
__global__ void k_vv1(int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* __restrict__ frc,
                      T dt, T dt2, const T* __restrict__ vcm, const double* __restrict__ cm_part, int n_cm_part, GridP<T> G) {
    T vc[3];
    const bool sub = pending_vcm<T>(vcm, cm_part, n_cm_part, vc);
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto v = vel[s]; auto p = pos[s]; auto f = frc[s];
        if (sub) cm_remove(v, vc);                                             // deferred remove_CM_motion!: the drift comes after it
        lone_kick(v, f, dt2);                                                  // :594
        drift(p, v, dt);                                                       // :602
        wrap_point(p.x, p.y, p.z, G);                                          // :609
        vel[s] = v; pos[s] = p;
    }
}

// fa (nullable): a second force array — the bonded sums + reciprocal-space forces of a small system's fused launches (step_fused.h) —
// folded in here; the total is written back so that the next first kick sees it
template <class T, bool CM>
__global__ void k_vv2(int64_t n, typename Vec<T>::T4* vel, typename Vec<T>::T4* frc, T dt2, double* cm_part,
                      const typename Vec<T>::T4* __restrict__ fa) {
    double px = 0, py = 0, pz = 0, m = 0;
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto v = vel[s]; auto f = frc[s];
        if (fa) { const auto g = fa[s]; f.x += g.x; f.y += g.y; f.z += g.z; }
        if (fa) frc[s] = f;
        lone_kick(v, f, dt2);                                                  // :616
        vel[s] = v;
        if constexpr (CM) { px += (double)v.x * v.w; py += (double)v.y * v.w; pz += (double)v.z * v.w; m += v.w; }
    }
    if constexpr (CM) block_cm_write(px, py, pz, m, cm_part);
}

// Second kick of step n and first kick + drift of step n+1 in ONE pass over the atoms (vv_run, single domain): halves the integrator's
// launches and its HBM traffic (48 B read + 32 B written per fp32 atom instead of 80 + 48).  remove_CM_motion! sits between the two
// kicks and needs Σ m v of ALL atoms, so it is applied one kernel late: this launch accumulates the partials of Σ m v_n (before the
// removal), carries on with the unshifted velocity, and the NEXT launch subtracts v_cm from the velocity it finds and v_cm·dt from
// the position that was drifted with it.  LAST: stop after the second kick (the run's final step), leaving v_n and x_n for the caller.
// TH (with LAST: the close launch of a step on which a rescaling thermostat applies, thermostat_step.h): one more per-block output, th_out =
// {Σ m|v|² of the velocities as stored, this block's share of the CSVR noise}.  The body is shared by two kernels: k_vv_mid, whose arguments and code
// are what they were, and k_vv_close, which carries the thermostat's.
template <class T, bool CM, bool LAST, bool TH>
__device__ __forceinline__ void vv_mid_body(int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* __restrict__ fr, T dt, T dt2,
                                            const double* __restrict__ cm_in, int n_cm_in, double* cm_out,
                                            const typename Vec<T>::T4* __restrict__ fa, const GridP<T>& G,
                                            const typename Vec<T>::T4* __restrict__ snap_a, const typename Vec<T>::T4* __restrict__ snap_b, float* trk_part,
                                            const ThermoP& th, double* th_out) {
    static_assert(!TH || LAST, "the thermostat's partials are taken by a launch that stops after the closing kick");
    const typename Vec<T>::T4* __restrict__ frc = fr;
    float v2m = 0.f, dam = 0.f, dbm = 0.f;      // of what this launch leaves behind
    // (The per-atom arithmetic and the Σ m v write of this body are written out: through per-atom helpers and block_cm_write the fp64 kernels took up to
    // 6 more VGPRs and 20 bytes of scratch, the fp32 one with CM 2 more VGPRs.)
    T vc[3] = {T(0), T(0), T(0)};
    const bool sub = cm_in != nullptr;
    // A lane's first atom is requested BEFORE the centre-of-mass partials are re-summed (32 KB of L2 reads, two barriers): the
    // streaming part of the launch then starts behind that latency instead of after it.
    using T4q = typename Vec<T>::T4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, sn = s;
    T4q vq = make4<T>(T(0), T(0), T(0), T(1)), fq = vq, pq = vq, gaq = vq;
    auto fetch = [&](int64_t a) {
        vq = vel[a]; fq = frc[a];
        if (!LAST || sub) pq = pos[a];
        if (fa) gaq = fa[a];
    };
    if (s < n) fetch(s);
    if (sub) block_vcm<T>(cm_in, n_cm_in, vc);
    const T sh[3] = {M<T>::mul(vc[0], dt), M<T>::mul(vc[1], dt), M<T>::mul(vc[2], dt)};
    double px = 0, py = 0, pz = 0, m = 0;
    [[maybe_unused]] double mv2 = 0;
    for (; s < n; s = sn) {
        sn = s + stride;
        const auto v0 = vq, f0 = fq, p0 = pq, ga0 = gaq;
        if (sn < n) fetch(sn);                                                 // the next atom's data travel while this one is integrated
        auto v = v0; auto f = f0; auto p = p0;
        if (fa) { f.x += ga0.x; f.y += ga0.y; f.z += ga0.z; }
        if (sub) {                                                             // remove_CM_motion! of the previous step, one launch late
            v.x -= vc[0]; v.y -= vc[1]; v.z -= vc[2];
            p.x = M<T>::sub(p.x, sh[0]); p.y = M<T>::sub(p.y, sh[1]); p.z = M<T>::sub(p.z, sh[2]);
        }
        const T kx = M<T>::mul(accel_of(f.x, v.w), dt2), ky = M<T>::mul(accel_of(f.y, v.w), dt2), kz = M<T>::mul(accel_of(f.z, v.w), dt2);
        v.x = M<T>::add(v.x, kx); v.y = M<T>::add(v.y, ky); v.z = M<T>::add(v.z, kz);   // :616, v_n before this step's CM removal
        if constexpr (CM) { px += (double)v.x * v.w; py += (double)v.y * v.w; pz += (double)v.z * v.w; m += v.w; }
        if constexpr (TH) thermo_accum<T>(v, mv2);
        if constexpr (!LAST) {
            v.x = M<T>::add(v.x, kx); v.y = M<T>::add(v.y, ky); v.z = M<T>::add(v.z, kz);   // :594 of the next step
            p.x = step_add(p.x, v.x, dt); p.y = step_add(p.y, v.y, dt); p.z = step_add(p.z, v.z, dt);   // :602
        }
        if (!LAST || sub) {
            wrap_point(p.x, p.y, p.z, G);                                      // :609
            pos[s] = p;
        }
        if (LAST && fa) const_cast<typename Vec<T>::T4*>(frc)[s] = f;  // the total force of the last step stays readable
        vel[s] = v;
        if (trk_part) {
            v2m = fmaxf(v2m, (float)(v.x * v.x + v.y * v.y + v.z * v.z));
            auto q = snap_a[s];
            T ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
            disp_image(ex, ey, ez, G);
            dam = fmaxf(dam, (float)(ex * ex + ey * ey + ez * ez));
            q = snap_b[s];
            ex = p.x - q.x; ey = p.y - q.y; ez = p.z - q.z;
            disp_image(ex, ey, ez, G);
            dbm = fmaxf(dbm, (float)(ex * ex + ey * ey + ez * ez));
        }
    }
    if (trk_part) block_trk_write(dam, dbm, v2m, trk_part);
    if constexpr (CM) {
        __shared__ double shm[4][4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { px += __shfl_xor(px, o, 64); py += __shfl_xor(py, o, 64); pz += __shfl_xor(pz, o, 64); m += __shfl_xor(m, o, 64); }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { shm[w][0] = px; shm[w][1] = py; shm[w][2] = pz; shm[w][3] = m; }
        __syncthreads();
        if (threadIdx.x < 4) { double a = 0; for (int q = 0; q < (int)(blockDim.x >> 6); ++q) a += shm[q][threadIdx.x]; cm_out[4 * (int64_t)blockIdx.x + threadIdx.x] = a; }
    }
    if constexpr (TH) thermo_write_partial(mv2, thermo_noise_share<T>(th), th_out);
}
template <class T, bool CM, bool LAST>
__global__ void k_vv_mid(int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* __restrict__ fr, T dt, T dt2,
                         const double* __restrict__ cm_in, int n_cm_in, double* cm_out,
                         const typename Vec<T>::T4* __restrict__ fa, GridP<T> G,
                         const typename Vec<T>::T4* __restrict__ snap_a = nullptr, const typename Vec<T>::T4* __restrict__ snap_b = nullptr, float* trk_part = nullptr) {
    vv_mid_body<T, CM, LAST, false>(n, pos, vel, fr, dt, dt2, cm_in, n_cm_in, cm_out, fa, G, snap_a, snap_b, trk_part, ThermoP{}, nullptr);
}
// the close launch of a coupled step: k_vv_mid<…, LAST> with the thermostat partials as one more output
template <class T, bool CM>
__global__ void k_vv_close(int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* __restrict__ fr, T dt, T dt2,
                           const double* __restrict__ cm_in, int n_cm_in, double* cm_out,
                           const typename Vec<T>::T4* __restrict__ fa, GridP<T> G, ThermoP th, double* th_out) {
    vv_mid_body<T, CM, true, true>(n, pos, vel, fr, dt, dt2, cm_in, n_cm_in, cm_out, fa, G, nullptr, nullptr, nullptr, th, th_out);
}

// the scale, then the first kick + drift + wrap of the next step and the maxima of the pair lists' validity check.
// No position shift: the drift happens after the removal.
template <class T>
__global__ void __launch_bounds__(256) k_vv_open(int64_t n, typename Vec<T>::T4* pos, typename Vec<T>::T4* vel, const typename Vec<T>::T4* __restrict__ frc, T dt, T dt2,
                                                 const double* __restrict__ cm_part, const double* __restrict__ th_part, int n_part, ThermoP P, GridP<T> G,
                                                 const typename Vec<T>::T4* __restrict__ snap_a, const typename Vec<T>::T4* __restrict__ snap_b, float* trk_part) {
    T vc[3];
    const T lam = thermo_block_lambda<T>(cm_part, th_part, n_part, P, vc);
    const bool sub = cm_part != nullptr;
    float v2m = 0.f, dam = 0.f, dbm = 0.f;
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto v = vel[s]; auto p = pos[s]; const auto f = frc[s];
        thermo_scale<T>(v, vc, sub, lam);
        lone_kick(v, f, dt2);                                                  // :594
        drift(p, v, dt);                                                       // :602
        wrap_point(p.x, p.y, p.z, G);                                          // :609
        vel[s] = v; pos[s] = p;
        if (trk_part) {      // (disp2_from written out: with it the fp32 kernel took 64 VGPRs instead of 50)
            v2m = fmaxf(v2m, (float)(v.x * v.x + v.y * v.y + v.z * v.z));
            auto q = snap_a[s];
            T ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
            disp_image(ex, ey, ez, G);
            dam = fmaxf(dam, (float)(ex * ex + ey * ey + ez * ez));
            q = snap_b[s];
            ex = p.x - q.x; ey = p.y - q.y; ez = p.z - q.z;
            disp_image(ex, ey, ez, G);
            dbm = fmaxf(dbm, (float)(ex * ex + ey * ey + ez * ez));
        }
    }
    if (trk_part) block_trk_write(dam, dbm, v2m, trk_part);
}

// frc += fa: the same fold outside the integrator
template <class T>
__global__ void k_add_forces(int64_t n, typename Vec<T>::T4* frc, const typename Vec<T>::T4* __restrict__ fa) {
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        auto f = frc[s];
        if (fa) { const auto g = fa[s]; f.x += g.x; f.y += g.y; f.z += g.z; }
        frc[s] = f;
    }
}

// Σ m v and Σ m of the current velocities (for an explicit remove_CM_motion! / multi-GPU all-reduce)
template <class T>
__global__ void k_cm_partials(int64_t n, const typename Vec<T>::T4* __restrict__ vel, const T* __restrict__ vcm, double* cm_part) {
    int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double px = 0, py = 0, pz = 0, m = 0;
    if (s < n) { auto v = vel[s]; if (vcm) cm_remove(v, vcm); px = (double)v.x * v.w; py = (double)v.y * v.w; pz = (double)v.z * v.w; m = v.w; }
    block_cm_write(px, py, pz, m, cm_part);
}

// one block of 256 threads: the partials' total → out4 = {Px,Py,Pz,M} (double), vcm = P/M (T)
template <class T>
__global__ void k_cm_finalize(int n_part, const double* __restrict__ cm_part, double* out4, T* vcm) {
    __shared__ double sh[4][4];
    double a[4];
    cm_partials_wave_sum(cm_part, n_part, a);
    if ((threadIdx.x & 63) == 0) for (int c = 0; c < 4; ++c) sh[threadIdx.x >> 6][c] = a[c];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0, 0, 0, 0};
        for (int q = 0; q < (int)(blockDim.x >> 6); ++q) for (int c = 0; c < 4; ++c) t[c] += sh[q][c];
        for (int c = 0; c < 4; ++c) out4[c] = t[c];
        if (vcm) for (int c = 0; c < 3; ++c) vcm[c] = (T)(t[c] / t[3]);
    }
}

// vcm = P/M from a device-resident {Px,Py,Pz,M} (the all-reduced total of a multi-GPU run)
template <class T>
__global__ void k_vcm_from_total(const double* __restrict__ total4, T* vcm) {
    if (threadIdx.x < 3) vcm[threadIdx.x] = (T)(total4[threadIdx.x] / total4[3]);
}

template <class T>
__global__ void k_shift_vel(int64_t n, typename Vec<T>::T4* vel, const T* __restrict__ vcm, const double* __restrict__ cm_part, int n_cm_part,
                            const int32_t* __restrict__ orig, const uint8_t* __restrict__ skip) {      // skip (nullable): per caller index, atoms left alone (virtual sites)
    T vc[3];
    pending_vcm<T>(vcm, cm_part, n_cm_part, vc);
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        if (orig && skip[orig[s]]) continue;
        auto v = vel[s]; cm_remove(v, vc); vel[s] = v;
    }
}

// the flush of a scale that the run's last step left pending (k_shift_vel's sibling); skip as there: a virtual site's velocity is left alone
template <class T>
__global__ void __launch_bounds__(256) k_scale_vel(int64_t n, typename Vec<T>::T4* vel, const double* __restrict__ cm_part, const double* __restrict__ th_part, int n_part, ThermoP P,
                                                   const int32_t* __restrict__ orig, const uint8_t* __restrict__ skip) {
    T vc[3];
    const T lam = thermo_block_lambda<T>(cm_part, th_part, n_part, P, vc);
    const bool sub = cm_part != nullptr;
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        if (orig && skip[orig[s]]) continue;
        auto v = vel[s];
        thermo_scale<T>(v, vc, sub, lam);
        vel[s] = v;
    }
}

// One atom's (m/2) v·v in double, every operation written out: vy², + vx² fused, + vz² fused, times m/2 — the form k_ke_partials has always been compiled to,
// pinned so that every kernel that takes the kinetic energy (k_ke_partials, k_record of record.h) gives the same bits whatever surrounds the expression.
template <class V4> __device__ inline double ke_atom(const V4& v) {
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
    return __dmul_rn(__dmul_rn((double)v.w, 0.5), __fma_rn(z, z, __fma_rn(x, x, __dmul_rn(y, y))));
}

// kinetic energy partials: Σ (m/2) v·v  (energy.jl:56-89)
template <class T>
__global__ void k_ke_partials(int64_t n, const typename Vec<T>::T4* __restrict__ vel, double* part) {
    int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double k = 0;
    if (s < n) { auto v = vel[s]; k = ke_atom(v); }
    __shared__ double sh[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) { double a = 0; for (int q = 0; q < (int)(blockDim.x >> 6); ++q) a += sh[q]; part[blockIdx.x] = a; }
}

// fixed-order sum of n doubles per block: block c sums part[c·n .. (c+1)·n) into out[c] (component-major partial arrays)
[[maybe_unused]] static __global__ void k_sum_double(int n, const double* __restrict__ part, double* out) {
    __shared__ double sh[256];
    part += (size_t)blockIdx.x * n;
    double a = 0;
    for (int q = threadIdx.x; q < n; q += blockDim.x) a += part[q];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int q = 0; q < (int)blockDim.x; ++q) t += sh[q]; out[blockIdx.x] = t; }
}

template <class T>
__global__ void k_check_finite(int64_t n, const typename Vec<T>::T4* __restrict__ pos, const typename Vec<T>::T4* __restrict__ vel,
                               const typename Vec<T>::T4* __restrict__ frc, int32_t* flags) {
    int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= n) return;
    auto p = pos[s]; auto v = vel[s]; auto f = frc[s];
    // every component on its own: in a sum +2e30 and −2e30 cancel, and nine components that are each in range add up to an alarm.  (NaN fails the comparison.)
    auto ok = [](T a) { return M<T>::fabs(a) <= T(1e30); };
    if (!(ok(p.x) && ok(p.y) && ok(p.z) && ok(v.x) && ok(v.y) && ok(v.z) && ok(f.x) && ok(f.y) && ok(f.z))) atomicOr(&flags[FLAG_NAN], 1);
}

}  // namespace mhip
