// ppcx_ppc_exact.hip -- gfx950 kernel of the exact posterior-predictive tail probabilities and interval per cell
// (ppcx_fit_ppc_exact, include/ppcx.h; the statistic: ppcx_ppc_exact.h, the negative-binomial tails: ppcx_nbcdf.h). The walk over
// the cells is ppcx_loo_dev.h's (for_gene_batches, for_given_columns); the drivers at the end of this file add the argument
// block and the kernel.
//
//   ppcx_ppc_exact_kernel  one workgroup of kBlockThreads per cell, a sibling of ppcx_loo_kernel. Pass 0 forms (eta_i, ln phi_i)
//                          of every draw once, from the transposed table T (ppcx_loo_table_kernel) or the given columns: 16
//                          bytes per draw, in LDS up to kPsisLdsDraws draws (64 KB: two workgroups per CU), in the workgroup's
//                          slice of a bounded global scratch beyond. Every later sweep (ppc_exact_sweeps, ppcx_ppc_exact.h, over
//                          ExactBlockSums of ppcx_loo_dev.h, as ppcx_loo_exact_kernel runs it) reads them strided and reduces with
//                          block_sum in the fixed order: the mean, the two variance sums, the two tails at y, and one sweep
//                          (two sums) per step of the quantile search, whose control flow is uniform because every thread
//                          holds the same sums. The draws of a wavefront run continued fractions of different lengths; the
//                          loop body is one division per half-step, selects for the guards and no transcendental
//                          (ppcx_nbcdf.h nb_beta_cf); the logarithms and exponentials of the prefactor are outside it, once
//                          per draw and sweep.
// Every reduction runs in a fixed order and a cell reads nothing of another cell: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_dev.h"
#include "ppcx_ppc_exact.h"

namespace ppcx {

struct PpcExactArgs {
  LooArgs l;                       // the table or the eta columns (l.cols), y, n, the cells, the scratch, out [cells][kPpcExactFields]
  const double* sgcols = nullptr;  // [cells][n] sigma_raw of the given columns (testing build)
  const int* ycols = nullptr;      // [cells] observed counts of the given columns
  double log_tc = 0.0, p_lo = 0.025, p_hi = 0.975;
};

// doubles per cell, in LDS or in the scratch: eta [n], ln phi [n]
__host__ __device__ inline long ppc_exact_slice(long n) { return 2 * n; }

template <bool LDS, bool COLS>
__global__ __launch_bounds__(kBlockThreads) void ppcx_ppc_exact_kernel(PpcExactArgs p) {
#pragma clang fp contract(off)
  extern __shared__ double lds_d[];
  __shared__ double red[kBlockWaves];
  const LooArgs& a = p.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  double* E = LDS ? lds_d : a.scratch + (long)blockIdx.x * ppc_exact_slice(n);   // [n] eta, then [n] ln phi (no selection arrays)
  double* LP = E + n;
  const LooCell c = loo_cell<COLS>(a, p.ycols);
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  double* o = a.out + (long)cell * kPpcExactFields;
  // ---- pass 0: (eta, ln phi) of every draw
  bool inval = false;
  {
    const double* Tg = COLS ? nullptr : a.T + (long)gi * (a.C + 1) * n;
    for (long i = tid; i < n; i += kBlockThreads) {
      const double eta = COLS ? a.cols[(long)cell * n + i] : loo_cell_eta(a, Tg, s, i);
      const double sg = COLS ? p.sgcols[(long)cell * n + i] : Tg[(long)a.C * n + i];
      const double lp = ppc_exact_lnphi(sg, p.log_tc);
      E[i] = eta; LP[i] = lp;
      inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
    }
  }
  if (block_any(inval)) { if (tid == 0) ppc_exact_store_nan(o, y, c.excluded); return; }   // a barrier: E, LP are visible
  // ---- the moments, the two tails at y, the interval: every sum unweighted and over n
  ppc_exact_sweeps(ExactBlockSums<false>{nullptr, E, LP, n, red}, y, c.excluded, n, p.p_lo, p.p_hi, tid == 0, o);
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_ppc_exact_kernel);
static hipError_t ppc_exact_cells(const PpcExactArgs& args, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  const long slice = ppc_exact_slice(args.l.n);
  return cells_in_batches(args, slice, n_cells, scratch_bytes, scratch, [&](const PpcExactArgs& p, const CellLaunch& c) {
    return launch_cell_kernel(pick_kernel<ppcx_ppc_exact_kernel_of>(c.lds, c.cols), p, c, 0, slice, st);
  });
}

hipError_t ppc_exact_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, double* out, size_t scratch_bytes,
                               hipStream_t st) {
  const double log_tc = log(tc);
  return for_gene_batches(fc, kPpcExactFields, out, scratch_bytes, st,
                          [&](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    PpcExactArgs p;
    p.l = a; p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi;
    return ppc_exact_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

hipError_t ppc_exact_columns(const GivenCells& gc, const double* sigma_raw, const int* y, double tc, double p_lo, double p_hi,
                             double* out, size_t scratch_bytes, hipStream_t st) {
  const size_t n_cols = (size_t)gc.n_cols;
  const double log_tc = log(tc);
  DeviceBuffer<double> d_sg; DeviceBuffer<int> d_y;      // outlive the walk, which drains the stream before it returns
  hipError_t e = d_sg.upload(sigma_raw, (size_t)gc.n * n_cols, st);
  if (e == hipSuccess) e = d_y.upload(y, n_cols, st);
  if (e != hipSuccess) return finish(e, st);
  return for_given_columns(gc, kPpcExactFields, out, st, [&](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    PpcExactArgs p;
    p.l = a; p.sgcols = d_sg.p; p.ycols = d_y.p; p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi;
    return ppc_exact_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

}  // namespace ppcx
