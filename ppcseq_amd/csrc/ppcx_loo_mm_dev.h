// ppcx_loo_mm_dev.h -- what the kernels over moment-matched cells share (ppcx_loo_mm.hip: the matching itself;
// ppcx_loo_mm_exact.hip: the exact predictive under the matched weights): the argument block of the matching, the gene a
// workgroup reads, and on the host what a walk of the matching keeps on the device beside for_gene_batches' own buffers, with
// the launch of plain PSIS-LOO and the matching over a batch of cells.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_loo_dev.h"
#include "ppcx_loo_mm.h"

namespace ppcx {

struct LooMmArgs {
  LooArgs l;                       // the table, y, r_eff, n, the cells, sel_pad, the scratch of both kernels (l.out: ppcx_loo_kernel's)
  const int* genes = nullptr;      // [table's genes] their ids in the model (device)
  const double* U = nullptr;       // [6][n] ppcx_loo_mm_hyper_kernel
  const double* loo = nullptr;     // [cells][kLooFields] ppcx_loo_kernel's fields of the table's cells
  int K = 0;                       // checked genes of the model
  double lambda_mu_mu = 0.0, k_threshold = 0.7;
  int max_iters = 0;
  double* out = nullptr;           // [cells][loo_mm_fields(C)]
};

// doubles per cell, in LDS or in the scratch: a candidate's ratios [n], the log weights [n], Q0 [n]
__host__ __device__ inline long loo_mm_slice(long n) { return 3 * n; }

// gene gi of the table as the local density reads it
__device__ __forceinline__ LooMmGene loo_mm_gene(const LooMmArgs& p, int gi) {
  const LooArgs& a = p.l;
  LooMmGene g;
  g.Tg = a.T + (long)gi * (a.C + 1) * a.n; g.U = p.U; g.n = a.n; g.C = a.C; g.S = a.S;
  g.checked = a.C >= 2 && p.genes[gi] < p.K;
  g.yrow = a.y + (long)gi * a.S; g.expo = a.expo; g.X = a.X; g.lambda_mu_mu = p.lambda_mu_mu;
  return g;
}

// ---- host (ppcx_loo_mm.hip)
// What a walk of the matching keeps for all of its gene batches: the draws' transposed hyper-parameters and ppcx_loo_kernel's
// fields of every cell. prepare() before for_gene_batches; args() once per gene batch, in the walk's order (it counts the cells
// of the earlier batches): the batch's LooMmArgs with the matching's record [cells][loo_mm_fields(C)] at `out` (device).
struct LooMmWalk {
  DeviceBuffer<double> U, loo;
  size_t done = 0;
  hipError_t prepare(const FitCells& fc, hipStream_t st);
  LooMmArgs args(const FitCells& fc, const LooArgs& a, const int* genes, int n_cells, double k_threshold, int max_iters, double* out);
};
// plain PSIS-LOO by its own kernel (its slices of the scratch lie within the matching's), then the matching, over the launch c
hipError_t launch_loo_mm_kernels(const LooMmArgs& q, const CellLaunch& c, hipStream_t st);

}  // namespace ppcx
