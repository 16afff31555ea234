// ppcx_reff.hip -- gfx950 kernel of the relative efficiency per observed cell (ppcx_fit_relative_eff, include/ppcx.h; the
// statistic: ppcx_reff.h).
//
//   ppcx_reff_kernel<LDS, COLS>  one workgroup per cell: the cell's log-likelihoods from the transposed gene table
//                                (ppcx_loo_table_kernel, loo_cell_ll) or, in the testing build, from host-given columns, written
//                                straight into split order; their maximum; v = exp(ll - max) in place; the Geyer ESS over the
//                                2 x chains sequences (summary_sequences, ppcx_summary_dev.h). LDS = true: the values live in LDS
//                                (8 bytes per split value, fits of up to kPsisLdsDraws draws); LDS = false: in the workgroup's
//                                slice of a bounded global scratch. No sort, no selection arrays.
// Every reduction runs in a fixed order and a cell reads nothing of another cell: its value is the same bits whatever genes are
// requested and however the work is batched.
#include <hip/hip_runtime.h>
#include "ppcx_summary_dev.h"
#include "ppcx_loo_dev.h"
#include "ppcx_reff.h"

namespace ppcx {

template <bool LDS, bool COLS>
__global__ __launch_bounds__(kBlockThreads) void ppcx_reff_kernel(ReffArgs a) {
  extern __shared__ double lds_z[];
  __shared__ SummaryShared sh;
  const int tid = threadIdx.x;
  const int nh = a.n_keep / 2, m = 2 * a.chains;
  const long N = (long)m * nh;
  const int cell = a.l.cell0 + blockIdx.x;              // of this launch's cells (the table's genes, or the given columns)
  double* out = a.l.out + cell;
  if (nh < 2) { if (tid == 0) *out = NAN; return; }
  double* Z = LDS ? lds_z : a.l.scratch + (long)blockIdx.x * N;   // [N] the split values
  int y = 0;
  if (!COLS) { const int ye = a.l.y[cell]; y = ye < 0 ? -ye - 1 : ye; }   // an excluded cell's log-likelihood is defined too
  const int gi = COLS ? 0 : cell / a.l.S, s = COLS ? 0 : cell - gi * a.l.S;
  bool bad = false; double lmax = -INFINITY;
  for (long k = tid; k < N; k += kBlockThreads) {
    const long j = split_source(k, nh, a.n_keep);
    const double ll = COLS ? a.l.cols[(long)cell * a.l.n + j] : loo_cell_ll(a.l, gi, s, j, y);
    bad = bad || isnan(ll) || ll == INFINITY;
    lmax = fmax(lmax, ll);
    Z[k] = ll;
  }
  bad = block_any(bad);
  if (bad) { if (tid == 0) *out = NAN; return; }
  const double L = block_max(lmax, sh.red);
  if (L == -INFINITY) { if (tid == 0) *out = NAN; return; }       // every value -Inf: all equal
  for (long k = tid; k < N; k += kBlockThreads) Z[k] = exp(Z[k] - L);   // each thread rewrites what it wrote
  __syncthreads();
  double ess = NAN;
  summary_sequences(Z, m, nh, true, &ess, sh);
  if (tid == 0) *out = ess / (double)N;
}

// ---- launch helpers (host)
static hipError_t launch_reff_kernel(const ReffArgs& a, int n_blocks, hipStream_t st) {
  const bool lds = a.l.n <= kPsisLdsDraws, cols = a.l.cols != nullptr;
  const size_t bytes = lds ? sizeof(double) * 2 * (size_t)a.chains * (size_t)(a.n_keep / 2) : 0;
  void (*const kernel)(ReffArgs) = lds ? (cols ? ppcx_reff_kernel<true, true> : ppcx_reff_kernel<true, false>)
                                       : (cols ? ppcx_reff_kernel<false, true> : ppcx_reff_kernel<false, false>);
  return launch_dynamic_lds(kernel, n_blocks, kBlockThreads, bytes, st, a);
}

// Cells of a launch in batches: all at once where the split values live in LDS, else as many as the scratch bound holds.
static hipError_t reff_cells(ReffArgs a, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  const long N = 2L * a.chains * (a.n_keep / 2);
  return loo_cell_batches(n_cells, a.l.n > kPsisLdsDraws ? N : 0, scratch_bytes, scratch, [&](int c0, int nc, double* scr) {
    a.l.cell0 = c0; a.l.scratch = scr;
    return launch_reff_kernel(a, nc, st);
  });
}

hipError_t reff_fit_cells(const double* draws, int chains, int n_keep, const Dims& d, const double* expo, const double* X, int n_genes,
                          const int* genes, const int* yenc, double* out, size_t scratch_bytes, hipStream_t st) {
  const int S = d.S, ncol = d.C + 1;
  const long n = (long)chains * n_keep;
  const size_t ncells = (size_t)n_genes * S;
  const int gb = column_batch(scratch_bytes, (long)ncol * n, n_genes);
  DeviceBuffer<int> d_genes, d_y; DeviceBuffer<double> d_T, d_out, d_scr;
  hipError_t e = d_genes.upload(genes, (size_t)n_genes, st);
  if (e == hipSuccess) e = d_y.upload(yenc, ncells, st);
  if (e == hipSuccess) e = d_out.alloc(ncells);
  if (e == hipSuccess) e = d_T.alloc((size_t)ncol * (size_t)n * gb);
  for (int g0 = 0; e == hipSuccess && g0 < n_genes; g0 += gb) {
    const int ng = n_genes - g0 < gb ? n_genes - g0 : gb;
    e = launch_loo_table_kernel(draws, n, d, d_genes.p + g0, ng, d_T.p, st);
    if (e != hipSuccess) break;
    ReffArgs a;
    a.chains = chains; a.n_keep = n_keep;
    a.l.T = d_T.p; a.l.y = d_y.p + (size_t)g0 * S; a.l.expo = expo; a.l.X = X; a.l.S = S; a.l.C = d.C; a.l.n = n;
    a.l.out = d_out.p + (size_t)g0 * S; a.l.n_cells = ng * S;
    e = reff_cells(a, ng * S, scratch_bytes, d_scr, st);
  }
  if (e == hipSuccess) e = d_out.download(out, ncells, st);
  return finish(e, st);
}

hipError_t reff_columns(const double* cols, int chains, int n_keep, int n_cols, double* out, size_t scratch_bytes, hipStream_t st) {
  const long n = (long)chains * n_keep;
  DeviceBuffer<double> d_cols, d_out, d_scr;
  hipError_t e = d_cols.upload(cols, (size_t)n * n_cols, st);
  if (e == hipSuccess) e = d_out.alloc((size_t)n_cols);
  if (e == hipSuccess) {
    ReffArgs a;
    a.chains = chains; a.n_keep = n_keep;
    a.l.cols = d_cols.p; a.l.n = n; a.l.n_cells = n_cols; a.l.out = d_out.p;
    e = reff_cells(a, n_cols, scratch_bytes, d_scr, st);
  }
  if (e == hipSuccess) e = d_out.download(out, (size_t)n_cols, st);
  return finish(e, st);
}

}  // namespace ppcx
