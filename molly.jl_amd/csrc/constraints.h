// constraints.h — SHAKE_RATTLE (constraints/shake.jl) inside the step loops of mhip_vv_run / mhip_langevin_run.
//
// The constraints are grouped into clusters on the host (build_clusters, constraints.jl:251-344): a central atom with 1, 2 or 3
// distance constraints to atoms of its own, or an angle constraint given as the triangle of its three distances.  On the device ONE
// lane owns a cluster and does, in registers, everything between two force passes that touches its atoms (k_con_step in
// constraints.hip): the kicks, RATTLE (shake.jl:512-715, one linear solve per cluster), the drift, SHAKE (the analytic root for two
// atoms, shake.jl:717-755; M-SHAKE — Newton on all constraints of the cluster at once — otherwise) with the velocity correction,
// the wrap.  Atoms outside every cluster are one-atom work items of the same grid.  The items are laid out by kind, each kind
// padded to a whole wave, so a wave never diverges on kind.  Atoms are addressed through inv[] (caller index → slot), so the
// engine's re-sorts need no remapping.
//
// The same lanes serve virtual sites (virtual_sites.h): a site whose parents are all atoms of one item is HOSTED by it — its force joins the
// parents' before the kick, its position is written behind the wrap.  Parents that are free atoms are joined into unconstrained groups for that.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "common.h"
#include "stochastic.h"
#include "thermostat.h"
#include "virtual_sites.h"

namespace mhip {

// work-item kinds, in layout order.  CK_G2..4: unconstrained groups — 2..4 free atoms joined into one item only because virtual sites hang off them
// (kicks, drift and wrap per atom, no solve); they exist only while sites are set
enum { CK_2 = 0, CK_3, CK_4, CK_ANGLE, CK_FREE, CK_G2, CK_G3, CK_G4, CK_N };
// one wave per workgroup: a lane's cluster solve is long and serial, so the 6mrr's ≈ 5 600 items are spread over ≈ 90 CUs instead of 22
constexpr int CON_BLOCK = 64;

// the clusters as the kernels see them: item t holds caller indices atoms[4t .. 4t+3] (−1: unused; −1 in the first: padding) and
// constraint lengths d[4t .. 4t+2]; a central-atom cluster has its centre first, an angle cluster is (i, j = centre, k) with
// d = (d_ij, d_jk, d_ik)
struct ClusterSet {
    std::vector<int32_t> atoms;
    std::vector<double> d;
    int32_t end[CK_N] = {};                // end of each kind's (padded) item range
    int64_t n_kind[4] = {0, 0, 0, 0};      // clusters of 2 / 3 / 4 atoms, angle clusters
    int64_t n_constraints = 0;             // degrees of freedom removed
    // hosted virtual sites (virtual_sites.h): a site whose parents are all atoms of ONE item is served by that item's lane.  Side table:
    // item t hosts the vs_item[2t + 1] sites from number vs_item[2t] on; site s is vs_rec[4s ..] = (type, caller index of the site atom,
    // local parent numbers l1 | l2 << 8 | l3 << 16, ·) with weights vs_w[6s ..].  A site atom is never an item of its own.
    std::vector<int32_t> vs_item, vs_rec;
    std::vector<double> vs_w;
    int64_t n_hosted = 0, n_host_items = 0, n_groups = 0;
    int64_t first_unhosted = -1;           // the first site no single item can host (parents in two clusters, or a union of free parents above four atoms)
    int32_t n_items() const { return end[CK_N - 1]; }
};
// throws ApiError{MHIP_ERR_INVALID} on what SHAKE_RATTLE cannot take: an atom in two clusters, more than three constraints on one
// centre, a chain, a ring, a linear angle, an index out of range, a non-positive length, a virtual site in a constraint (virtual.jl:174-178)
ClusterSet build_clusters(int64_t n_atoms, int64_t n_dist, const int32_t* i, const int32_t* j, const double* dist,
                          int64_t n_angle, const int32_t* ai, const int32_t* aj, const int32_t* ak, const double* d3, const SiteSet* vs = nullptr);

template <class T> struct ConP {
    const int32_t* atoms; const double* d; const int32_t* inv;
    int32_t end[CK_N];
    double tol;                    // SHAKE: | |r| − d | <= tol for every constraint of the cluster
    int32_t max_iters;
    unsigned long long* stat;      // [0] += cluster-solves that stopped at max_iters, [1] = max(iterations any cluster took)
    const int32_t* vs_item; const int32_t* vs_rec; const double* vs_w;      // hosted virtual sites (null: none)
};

// what one launch reads and writes besides the clusters
template <class T> struct ConStep {
    using T4 = typename Vec<T>::T4;
    T4* pos; T4* vel; const T4* frc; const T4* fa;      // fa (nullable): a side force array added on the way (a small system's bonded sums)
    const T* vcm; const double* cm_in; int n_cm_in;     // the pending Σ m v removal (PendingCm): a vcm, or per-block partials to re-sum
    double* cm_out;                                     // nullable: this launch's Σ m v partials, one per block
    const T4* snap_a; const T4* snap_b; float* trk_part; // nullable: the validity check of the pair lists (as k_vv_mid measures it)
    T dt, dt2;
    StochP<T> S;                                        // Langevin only
};

// n_blocks <= 1024 workgroups of CON_BLOCK lanes (the Σ m v partials fill at most one half of the engine's cm_step)
// mode 0: first kick + RATTLE + drift + SHAKE (the first step of mhip_vv_run, k_vv1's place); 1: closing kick + RATTLE, Σ m v, then
// the next step's kick + RATTLE + drift + SHAKE (k_vv_mid's place); 2: closing kick + RATTLE, Σ m v (the run's last step); 3: the
// Langevin step after the forces (k_langevin's place)
template <class T>
void launch_con_step(hipStream_t s, int n_blocks, int mode, const ConP<T>& C, const ConStep<T>& A, const GridP<T>& G, const ThermoArgs* X = nullptr);
// X (nullable): a step on which a rescaling thermostat applies (thermostat_step.h), launched as k_con_thermo with one more kernel argument — mode 2 is its close launch
// and leaves the thermostat partials in X->th_out, mode 0 its open launch and reads them (X->th_in) beside A.cm_in.  The uncoupled launches' arguments are what they were.

// The constraint contribution to the virial at the state held (mhip_constraint_virial): the reference's trial step — RATTLE, kick by dt + RATTLE, drift by dt +
// SHAKE (merge_initial_constraint_virial!, simulators.jl:459-495) — per cluster in double, read-only.  f: the total forces, caller order, packed xyz; lam
// (nullable: 1): the per-atom λ, caller order; part: 19 component-major runs of n_blocks partials (Wv[9], Wp[9], the solves that stopped at max_iters).
template <class T> struct ConVirial {
    using T4 = typename Vec<T>::T4;
    const T4* pos; const T4* vel; const T* f; const T* lam;
    double dt;
    double* part;
};
// n_blocks <= 1024 workgroups of CON_BLOCK lanes over the items [0, C.end[CK_ANGLE]); C.stat and the hosted sites are not read
template <class T>
void launch_con_virial(hipStream_t s, int n_blocks, const ConP<T>& C, const ConVirial<T>& A, const GridP<T>& G);

}  // namespace mhip
