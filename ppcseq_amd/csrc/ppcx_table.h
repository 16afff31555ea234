// ppcx_table.h -- the transposed table of per-draw parameters T[g][c][draw] that the per-cell kernels read (ppcx_ppc.hip:
// ppcx_ppc_table_kernel; ppcx_loo.hip: ppcx_loo_table_kernel, for every kernel over ppcx_loo_dev.h): how it is built and how a
// cell reads a draw from it. Rows c = 0 intercept, 1 .. C - 1 slopes (0 for a gene without slopes), C the dispersion -- the
// per-gene work done once per draw instead of once per draw and sample, and a wavefront's lanes read consecutive draws of one
// parameter. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_model.h"
#include "ppcx_ppc.h"

namespace ppcx {

// The body of a table kernel: one thread per (draw j, gene gi of the table), 256 threads, grid (draws / 32, genes / 32); 32 x 32
// tiles through LDS so that both the reads (along the genes) and the writes (along the draws) are coalesced. genes: the table's
// genes in the model (null: the first n_genes). PHI: the last row holds phi = ppc_phi(sigma_raw, tc), else sigma_raw itself.
template <bool PHI>
__device__ __forceinline__ void table_tiles(const double* draws, long n_draws, const Dims& d, const int* genes, int n_genes, double tc,
                                            double* T) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
  const long j0 = (long)blockIdx.x * 32; const int g0 = blockIdx.y * 32;
  const int ncol = d.C + 1;
  for (int c = 0; c < ncol; ++c) {
    for (int r = ty; r < 32; r += 8) {
      const long j = j0 + r; const int gi = g0 + tx;
      double v = 0.0;
      if (j < n_draws && gi < n_genes) {
        const double* u = draws + j * (long)d.D;
        const int g = genes ? genes[gi] : gi;
        if (c == 0) v = u[d.off_intercept + g];
        else if (c < d.C) v = g < d.K ? u[coef_index(d, c, g)] : 0.0;
        else v = PHI ? ppc_phi(u[d.off_sigma_raw + g], tc) : u[d.off_sigma_raw + g];
      }
      tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int gi = g0 + r; const long j = j0 + tx;
      if (j < n_draws && gi < n_genes) T[((long)gi * ncol + c) * n_draws + j] = tile[tx][r];
    }
    __syncthreads();
  }
}

// Draw j of a cell of sample s from its gene's rows Tg = T + gi (C + 1) n: the linear predictor eta = expo + sum_c X_sc T_c and
// the last row's entry (phi or sigma_raw). expo = exposure[s]; X [C][S].
__device__ __forceinline__ void table_draw(const double* Tg, long n, int C, double expo, const double* X, int S, int s, long j,
                                           double* eta_out, double* last_out) {
  double eta = expo + X[s] * Tg[j];
  for (int cc = 1; cc < C; ++cc) eta += X[(long)cc * S + s] * Tg[(long)cc * n + j];
  *eta_out = eta; *last_out = Tg[(long)C * n + j];
}

}  // namespace ppcx
