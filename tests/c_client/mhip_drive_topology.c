/* mhip_drive_topology.c — a plain C99 client of libmollyhip.so that makes the set-up calls the Julia shim (julia/ext/MollyHIPExt.jl) makes for a
 * real protein, in the shim's order, on inputs read from a file:
 *
 *   mhip_create → mhip_set_atoms → mhip_set_exceptions → mhip_set_bonds → mhip_set_angles → mhip_set_torsions → mhip_set_ewald_exclusions
 *   → mhip_set_pme → mhip_set_state → mhip_export_neighbors (count, then fill) → mhip_forces + mhip_specific_forces + mhip_general_forces
 *   (accumulating into one buffer) → the three potential energies → mhip_remove_cm → mhip_random_velocities → mhip_langevin_run
 *   → mhip_get_state → mhip_destroy
 *
 * tests/test_gpu_c_client.py writes the input (6mrr with bonded terms and PME, fp64), compiles this file with gcc, runs it on the GPU box and checks
 * the output against the oracle and OpenMM.  Usage: mhip_drive_topology <in.bin> <out.bin>
 *
 * in.bin:  uint64 hdr[20] — 0 sizeof(mhip_config), 1 n, 2 n_excluded, 3 n_special, 4 n_bonds, 5 n_angles, 6 n_torsion_terms, 7 n_ewald_exclusions,
 *                           8 PME order, 9-11 PME mesh, 12 Langevin steps, 13 random_velocities key, 14 its ctr1, 15 Langevin key, 16 its ctr1
 *          double dh[8] — 0 PME α, 1 ϵr, 2 kT of random_velocities, 3 dt, 4 kT of the Langevin run, 5 friction
 *          the mhip_config bytes; x[3n], v[3n], charge[n], sigma[n], eps[n], mass[n] (double); excluded i[], j[]; special i[], j[] (int32);
 *          bonds i[], j[] (int32), k[], r0[] (double); angles i[], j[], k[] (int32), kθ[], θ0[]; torsions i[], j[], k[], l[], periodicity[]
 *          (int32), phase[], k[]; Ewald exclusions i[], j[] (int32)
 * out.bin: int64 n_pairs; int32 i[n_pairs], j[n_pairs]; uint8 special[n_pairs]; double f[3n], pe_pair, pe_specific, pe_general,
 *          v after mhip_remove_cm [3n], v after mhip_random_velocities [3n], x and v after the Langevin run [3n] each
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mollyhip.h"

#define CHECK(call) do { int32_t rc_ = (call); if (rc_ != MHIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, (int)rc_, mhip_last_error(ctx)); return 2; } } while (0)

static FILE* fin;
static void* take(size_t bytes) {   /* the next `bytes` of the input, in a fresh allocation (NULL for 0 bytes) */
    if (bytes == 0) return NULL;
    void* p = malloc(bytes);
    if (!p || fread(p, 1, bytes, fin) != bytes) { fprintf(stderr, "input file too short\n"); exit(1); }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    fin = fopen(argv[1], "rb");
    if (!fin) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    uint64_t* hdr = take(20 * sizeof(uint64_t));
    double* dh = take(8 * sizeof(double));
    if (hdr[0] != sizeof(mhip_config)) { fprintf(stderr, "mhip_config is %zu bytes here, %llu in the input\n", sizeof(mhip_config), (unsigned long long)hdr[0]); return 1; }
    mhip_config* cfg = take(sizeof(mhip_config));
    const int64_t n = (int64_t)hdr[1], n_ex = (int64_t)hdr[2], n_sp = (int64_t)hdr[3], n_b = (int64_t)hdr[4], n_a = (int64_t)hdr[5], n_t = (int64_t)hdr[6], n_ew = (int64_t)hdr[7];
    const size_t d3 = 3 * (size_t)n * sizeof(double), d1 = (size_t)n * sizeof(double), i4 = sizeof(int32_t), f8 = sizeof(double);
    double *x = take(d3), *v = take(d3), *q = take(d1), *sigma = take(d1), *eps = take(d1), *mass = take(d1);
    int32_t *ex_i = take(n_ex * i4), *ex_j = take(n_ex * i4), *sp_i = take(n_sp * i4), *sp_j = take(n_sp * i4);
    int32_t *b_i = take(n_b * i4), *b_j = take(n_b * i4); double *b_k = take(n_b * f8), *b_r0 = take(n_b * f8);
    int32_t *a_i = take(n_a * i4), *a_j = take(n_a * i4), *a_k = take(n_a * i4); double *a_kth = take(n_a * f8), *a_th0 = take(n_a * f8);
    int32_t *t_i = take(n_t * i4), *t_j = take(n_t * i4), *t_k = take(n_t * i4), *t_l = take(n_t * i4), *t_per = take(n_t * i4);
    double *t_ph = take(n_t * f8), *t_k0 = take(n_t * f8);
    int32_t *w_i = take(n_ew * i4), *w_j = take(n_ew * i4);
    if (fgetc(fin) != EOF) { fprintf(stderr, "input file longer than its header says\n"); return 1; }
    fclose(fin);
    const int32_t mesh[3] = {(int32_t)hdr[9], (int32_t)hdr[10], (int32_t)hdr[11]};
    double *f = calloc(3 * (size_t)n, sizeof(double)), *v_cm = malloc(d3), *v_rand = malloc(d3), *x_end = malloc(d3), *v_end = malloc(d3);
    if (!f || !v_cm || !v_rand || !x_end || !v_end) return 1;

    mhip_ctx* ctx = NULL;
    int32_t rc = mhip_create(&ctx, cfg);
    if (rc != MHIP_OK) { fprintf(stderr, "mhip_create failed: %d (%s)\n", (int)rc, mhip_last_error(NULL)); return 2; }
    CHECK(mhip_set_atoms(ctx, q, sigma, eps, mass, NULL, MHIP_MEM_HOST));
    CHECK(mhip_set_exceptions(ctx, ex_i, ex_j, n_ex, sp_i, sp_j, n_sp));
    CHECK(mhip_set_bonds(ctx, n_b, b_i, b_j, b_k, b_r0));
    CHECK(mhip_set_angles(ctx, n_a, a_i, a_j, a_k, a_kth, a_th0));
    CHECK(mhip_set_torsions(ctx, n_t, t_i, t_j, t_k, t_l, t_per, t_ph, t_k0));
    CHECK(mhip_set_ewald_exclusions(ctx, n_ew, w_i, w_j));
    CHECK(mhip_set_pme(ctx, (int32_t)hdr[8], mesh, dh[0], dh[1]));
    CHECK(mhip_set_state(ctx, x, v, MHIP_MEM_HOST));

    /* the neighbour export: ask for the count with no buffers, then fill */
    int64_t n_pairs = 0;
    CHECK(mhip_export_neighbors(ctx, NULL, NULL, NULL, 0, &n_pairs));
    int32_t *pi = malloc((size_t)(n_pairs ? n_pairs : 1) * i4), *pj = malloc((size_t)(n_pairs ? n_pairs : 1) * i4);
    uint8_t* psp = malloc((size_t)(n_pairs ? n_pairs : 1));
    if (!pi || !pj || !psp) return 1;
    int64_t n_filled = 0;
    CHECK(mhip_export_neighbors(ctx, pi, pj, psp, n_pairs, &n_filled));
    if (n_filled != n_pairs) { fprintf(stderr, "export_neighbors: %lld pairs counted, %lld filled\n", (long long)n_pairs, (long long)n_filled); return 3; }

    /* forces! (force.jl:792-795, 1228-1231): every part accumulates into the caller's zeroed buffer */
    CHECK(mhip_forces(ctx, 0, 1, f, NULL, MHIP_MEM_HOST));
    CHECK(mhip_specific_forces(ctx, 1, f, MHIP_MEM_HOST));
    CHECK(mhip_general_forces(ctx, 1, f, MHIP_MEM_HOST));
    double pe[3] = {0, 0, 0};
    CHECK(mhip_potential_energy(ctx, 0, &pe[0]));
    CHECK(mhip_specific_potential_energy(ctx, &pe[1]));
    CHECK(mhip_general_potential_energy(ctx, &pe[2]));

    CHECK(mhip_remove_cm(ctx));
    CHECK(mhip_get_state(ctx, NULL, v_cm, MHIP_MEM_HOST));
    CHECK(mhip_random_velocities(ctx, dh[2], hdr[13], hdr[14]));
    CHECK(mhip_get_state(ctx, NULL, v_rand, MHIP_MEM_HOST));
    CHECK(mhip_langevin_run(ctx, 0, (int64_t)hdr[12], dh[3], dh[4], dh[5], 1, hdr[15], hdr[16]));
    CHECK(mhip_get_state(ctx, x_end, v_end, MHIP_MEM_HOST));
    CHECK(mhip_destroy(ctx));

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    fwrite(&n_pairs, sizeof n_pairs, 1, fo);
    fwrite(pi, i4, (size_t)n_pairs, fo); fwrite(pj, i4, (size_t)n_pairs, fo); fwrite(psp, 1, (size_t)n_pairs, fo);
    fwrite(f, f8, 3 * (size_t)n, fo); fwrite(pe, f8, 3, fo);
    fwrite(v_cm, f8, 3 * (size_t)n, fo); fwrite(v_rand, f8, 3 * (size_t)n, fo); fwrite(x_end, f8, 3 * (size_t)n, fo); fwrite(v_end, f8, 3 * (size_t)n, fo);
    if (fclose(fo) != 0) return 1;
    return 0;
}
