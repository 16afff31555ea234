// ppcx_reff.hip -- gfx950 kernel of the relative efficiency per observed cell (ppcx_fit_relative_eff, include/ppcx.h; the
// statistic: ppcx_reff.h). The walk over the cells is ppcx_loo_dev.h's (for_gene_batches, for_given_columns); the drivers at the
// end of this file add the argument block and the kernel.
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
  const LooCell c = loo_cell<COLS>(a.l);                // an excluded cell's log-likelihood is defined too
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  double* out = a.l.out + cell;
  if (nh < 2) { if (tid == 0) *out = NAN; return; }
  double* Z = LDS ? lds_z : a.l.scratch + (long)blockIdx.x * N;   // [N] the split values
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
PPCX_KERNEL_OF(ppcx_reff_kernel);
// the split values of a cell [2 chains (n_keep / 2)]: its slice, in LDS or in the scratch (no selection arrays)
static hipError_t reff_cells(const ReffArgs& args, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  const long N = 2L * args.chains * (args.n_keep / 2);
  return cells_in_batches(args, N, n_cells, scratch_bytes, scratch, [&](const ReffArgs& a, const CellLaunch& c) {
    return launch_cell_kernel(pick_kernel<ppcx_reff_kernel_of>(c.lds, c.cols), a, c, 0, N, st);
  });
}

// what both walks run per batch: the kernel over the batch's cells
static auto reff_body(int chains, int n_keep, size_t scratch_bytes, hipStream_t st) {
  return [=](const LooArgs& l, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    ReffArgs a;
    a.l = l; a.chains = chains; a.n_keep = n_keep;
    return reff_cells(a, n_cells, scratch_bytes, scratch, st);
  };
}
hipError_t reff_fit_cells(const FitCells& fc, double* out, size_t scratch_bytes, hipStream_t st) {
  return for_gene_batches(fc, 1, out, scratch_bytes, st, reff_body(fc.chains, fc.n_keep, scratch_bytes, st));
}
hipError_t reff_columns(const GivenCells& gc, double* out, size_t scratch_bytes, hipStream_t st) {
  return for_given_columns(gc, 1, out, st, reff_body(gc.chains, gc.n_keep, scratch_bytes, st));
}

}  // namespace ppcx
