// ppcx_loo_exact.hip -- gfx950 kernel of the exact leave-one-out predictive tail probabilities and interval per cell
// (ppcx_fit_loo_predict_exact, ppcx_fit_loo_predict_exact_approx, include/ppcx.h; the statistic: ppcx_loo_exact.h, the weights:
// ppcx_loo_dev.h, the negative-binomial tails: ppcx_nbcdf.h). The walk over the cells is ppcx_loo_dev.h's (for_gene_batches,
// for_given_columns); the drivers at the end of this file add the argument block and the kernel. The kernel's body is
// loo_exact_cell (ppcx_loo_dev.h), which the moment-matched kernels call for their unmatched cells.
//
//   ppcx_loo_exact_kernel  one workgroup of kBlockThreads per cell, a sibling of ppcx_loo_predict_kernel (the weights) and of
//                          ppcx_ppc_exact_kernel (everything after them). The cell's ratios from the transposed table T
//                          (ppcx_loo_table_kernel) or the given columns, the tail and the normalised weights by loo_cell_weights
//                          (ppcx_loo_dev.h), which ppcx_loo_predict_kernel calls too: khat is its khat bit for bit. The ratios
//                          are dead once the weights exist; only then (eta_i, ln phi_i) of every draw are formed, eta into the
//                          ratios' place (the table is therefore read twice per draw, as ppcx_loo_predict_kernel reads it for
//                          its counts). Every later sweep (ppc_exact_sweeps, ppcx_ppc_exact.h, over ExactBlockSums) reads
//                          (w_i, eta_i, ln phi_i) strided and reduces with block_sum in the fixed order: the mean, the two
//                          variance sums, the two tails at y, and one sweep (two sums) per step of each quantile search,
//                          whose control flow is uniform because every thread holds the same sums.
//                          A cell that a NUTS fit excludes runs the same sweeps with w_i = 1 and every sum divided by n
//                          (ppcx_loo_exact.h step 5): ppcx_ppc_exact_kernel's bits, by the same template.
//                          AP: the ratios of an ADVI fit, (log_p - log_g) - ll; an excluded cell weighted by log_p - log_g.
//                          Per draw 24 bytes in three arrays -- ratio then eta (8), log weight then weight (8), ln phi (8) --
//                          in LDS up to kPsisLdsDraws draws, beside the two selection arrays (16 bytes per slot of
//                          loo_sel_pad: 4 KB at 4 096 draws and r_eff = 1), in the workgroup's slice of a bounded global scratch
//                          beyond. At 4 096 draws that is 96 KB + 4 KB + 2.8 KB static: ONE workgroup per CU of 160 KB, as
//                          four arrays (128 KB) would give; the third array's saving shows below 3 100 draws, where two
//                          workgroups fit (four arrays: below 2 300), three below 2 000; a fit of 1 000 draws takes 26 KB and
//                          the registers bind first (146 VGPRs: three workgroups per CU). The layout was
//                          chosen on this arithmetic alone: the four-array form has NOT been timed against it (the entry's
//                          time as it is: profiles/README.md, cell_entries_ab.json).
// Every reduction runs in a fixed order and a cell reads nothing of another cell: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_dev.h"
#include "ppcx_loo_exact.h"

namespace ppcx {

struct LooExactArgs {
  LooArgs l;                       // the table or the ll columns (l.cols), y, r_eff, lr, n, the cells, sel_pad, the scratch, out [cells][kLooExactFields]
  const double* etacols = nullptr; // [cells][n] linear predictors of the given columns (testing build)
  const double* sgcols = nullptr;  // [cells][n] sigma_raw of the given columns
  const int* ycols = nullptr;      // [cells] observed counts of the given columns
  double log_tc = 0.0, p_lo = 0.025, p_hi = 0.975;
};

// AP: the weights of an ADVI fit (ppcx_loo_ap.h). The stages are loo_exact_cell's (ppcx_loo_dev.h), which the moment-matched
// kernels run on their unmatched cells.
template <bool LDS, bool COLS, bool AP>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_exact_kernel(LooExactArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  const LooArgs& a = p.l;
  const LooCell c = loo_cell<COLS>(a, p.ycols);
  loo_exact_cell<COLS, AP>(a, c, cell_mem<LDS>(lds_u, a, loo_slice3(a.n)), p.etacols, p.sgcols, p.log_tc, p.p_lo, p.p_hi,
                           a.out + (long)c.cell * kLooExactFields, sh);
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_exact_kernel);
static hipError_t loo_exact_cells(const LooExactArgs& args, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  const long slice = loo_slice3(args.l.n);
  return cells_in_batches(args, slice, n_cells, scratch_bytes, scratch, [&](const LooExactArgs& p, const CellLaunch& c) {
    return launch_cell_kernel(pick_kernel<ppcx_loo_exact_kernel_of>(c.lds, c.cols, p.l.lr != nullptr), p, c, p.l.sel_pad, slice, st);
  });
}

// a NUTS fit (fc.log_ratio null) or an ADVI fit (fc.log_ratio: log_p - log_g of the draws)
hipError_t loo_exact_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, double* out, size_t scratch_bytes,
                               hipStream_t st) {
  const double log_tc = log(tc);
  return for_gene_batches(fc, kLooExactFields, out, scratch_bytes, st,
                          [&](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    LooExactArgs p;
    p.l = a; p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi;
    return loo_exact_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

hipError_t loo_exact_columns(const GivenCells& gc, const double* eta, const double* sigma_raw, const int* y, double tc, double p_lo,
                             double p_hi, double* out, size_t scratch_bytes, hipStream_t st) {
  const size_t n_cols = (size_t)gc.n_cols;
  const double log_tc = log(tc);
  DeviceBuffer<double> d_eta, d_sg; DeviceBuffer<int> d_y;   // outlive the walk, which drains the stream before it returns
  hipError_t e = d_eta.upload(eta, (size_t)gc.n * n_cols, st);
  if (e == hipSuccess) e = d_sg.upload(sigma_raw, (size_t)gc.n * n_cols, st);
  if (e == hipSuccess) e = d_y.upload(y, n_cols, st);
  if (e != hipSuccess) return finish(e, st);
  return for_given_columns(gc, kLooExactFields, out, st, [&](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    LooExactArgs p;
    p.l = a; p.etacols = d_eta.p; p.sgcols = d_sg.p; p.ycols = d_y.p; p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi;
    return loo_exact_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

}  // namespace ppcx
