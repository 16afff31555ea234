// ppcx_loo_predict.hip -- gfx950 kernel of the leave-one-out predictive interval and LOO-PIT per observed cell
// (ppcx_fit_loo_predict, include/ppcx.h; the statistic: ppcx_loo_predict.h). The walk over the cells is ppcx_loo_dev.h's
// (for_gene_batches, for_given_columns); the drivers at the end of this file add the argument block and the kernel.
//
//   ppcx_loo_predict_kernel  one workgroup of kBlockThreads per cell. The cell's n ratios r = -ll from the transposed table T
//                            (ppcx_loo_table_kernel) and its tail as in ppcx_loo_kernel (ppcx_loo_dev.h); then per draw its
//                            predictive count x_i (nb2_log_rng on the address of ppcx_fit_ppc) and its weight w_i: the tail
//                            position of a draw by binary search in the sorted keys of the M + 1 largest ratios, and for keys
//                            that occur more than once a scan of the earlier draws (the tie rule of ppcx_loo_predict.h). Sums of
//                            weights give the mean and the two ends of the LOO-PIT; each quantile is a bisection on the integer
//                            value with one fixed-order sum of weights per step.
//                            Per draw 20 bytes: r (8), w (8), x (4) -- in LDS up to kPsisLdsDraws draws (80 KB, beside the two
//                            selection arrays), in the workgroup's slice of a bounded global scratch beyond.
//                            AP (ppcx_fit_loo_predict_approx): the ratios of an ADVI fit, (log_p - log_g) - ll, and an excluded
//                            cell down the weighted path with log_p - log_g (ppcx_loo_ap.h); the rest is the same code.
// Every reduction runs in a fixed order and a cell reads nothing of another cell: its fields are the same bits whatever else is
// requested and however the work is batched. Neither the log-likelihood nor the counts matrix is materialised.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "ppcx_loo_dev.h"
#include "ppcx_loo_predict.h"

namespace ppcx {

struct LooPredictArgs {
  LooArgs l;                       // the table or the columns, y, r_eff, n, the cells, sel_pad, the scratch, out [cells][kLooPredictFields]
  const int* genes = nullptr;      // [table's genes] their ids in the model: the Philox address is genes[gi] S + s
  const int* xcols = nullptr;      // [cells][n] predictive counts of the given columns (testing build)
  const int* ycols = nullptr;      // [cells] observed counts of the given columns
  double tc = 1.0, p_lo = 0.025, p_hi = 0.975;
  uint32_t k0 = 0;
};

// doubles per cell, in LDS or in the scratch: r [n], w [n], x [n] as integers
__host__ __device__ inline long loo_predict_slice(long n) { return 2 * n + (n + 1) / 2; }

// AP: the weights of an ADVI fit (ppcx_loo_ap.h: ratios (log_p - log_g) - ll; an excluded cell is weighted too, by log_p - log_g)
template <bool LDS, bool COLS, bool AP>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_predict_kernel(LooPredictArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  const LooArgs& a = p.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_predict_slice(n));
  double* V = m.V;                                       // [n] the ratios r = -ll
  double* W = V + n;                                     // [n] log weights, then weights
  int* XI = reinterpret_cast<int*>(W + n);               // [n] predictive counts
  const LooCell c = loo_cell<COLS>(a, p.ycols);
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  double* o = a.out + (long)cell * kLooPredictFields;
  auto all_nan = [&]() { if (tid == 0) for (int f = 0; f < kLooPredictFields; ++f) o[f] = NAN; };
  // ---- the ratios
  CellRatios cr;
  const CellVerdict verdict = loo_cell_verdict<COLS, AP>(a, c, m, nullptr, sh, &cr);
  if (verdict == CELL_NAN) { all_nan(); return; }
  // ---- the predictive count of every draw
  bool inval = false;
  if (COLS) {
    for (long i = tid; i < n; i += kBlockThreads) { const int v = p.xcols[(long)cell * n + i]; XI[i] = v; inval = inval || v == kPpcInvalid; }
  } else {
    const double* Tg = a.T + (long)gi * (a.C + 1) * n;
    const uint32_t addr = ppc_cell_address(p.genes[gi], a.S, s);
    for (long i = tid; i < n; i += kBlockThreads) {
      double sigma_raw;
      const double eta = loo_cell_eta(a, Tg, s, i, &sigma_raw);
      const int v = nb2_log_rng(eta, ppc_phi(sigma_raw, p.tc), p.k0, addr, (uint32_t)i);
      XI[i] = v; inval = inval || v == kPpcInvalid;
    }
  }
  if (block_any(inval)) { all_nan(); return; }           // block_any: XI is visible to every thread
  const double pr[2] = {p.p_lo, p.p_hi};
  double q[2];
  if (verdict == CELL_UNIFORM) {
    // ---- already held out: uniform weights over all n draws, the type-7 quantiles of the posterior-predictive kernels
    const double sum = draws_sum(n, sh.red, [&](long i) { return (double)XI[i]; });
    const int vmax = (int)draws_max(n, sh.red, [&](long i) { return (double)XI[i]; });
    auto count_le = [&](int v) { return (long)draws_sum(n, sh.red, [&](long i) { return XI[i] <= v ? 1.0 : 0.0; }); };
    auto min_above = [&](int v) { return (int)-draws_max(n, sh.red, [&](long i) { return XI[i] > v ? -(double)XI[i] : -INFINITY; }); };
    for (int k = 0; k < 2; ++k) {
      double h; long r; int v0, v1;
      type7_rank(n, pr[k], &h, &r);
      select_pair(n, r, vmax, count_le, min_above, &v0, &v1);
      q[k] = type7(h, r, n, (double)v0, (double)v1);
    }
    const double lt = draws_sum(n, sh.red, [&](long i) { return XI[i] < y ? 1.0 : 0.0; });
    const double le = draws_sum(n, sh.red, [&](long i) { return XI[i] <= y ? 1.0 : 0.0; });
    if (tid == 0) { o[0] = sum / (double)n; o[1] = q[0]; o[2] = q[1]; o[3] = lt / (double)n; o[4] = le / (double)n; o[5] = NAN; }
    return;
  }
  // ---- the tail, and the normalised weight of every draw
  const double khat = loo_cell_weights<true>(a, c, m, cr, W, sh);
  __syncthreads();
  // ---- sums of weights: the mean, the LOO-PIT, and F for the quantiles (a draw that takes no part has weight 0)
  const double mean = draws_sum(n, sh.red, [&](long i) { return W[i] * (double)XI[i]; });
  const double plt = draws_sum(n, sh.red, [&](long i) { return XI[i] < y ? W[i] : 0.0; });
  const double ple = draws_sum(n, sh.red, [&](long i) { return XI[i] <= y ? W[i] : 0.0; });
  auto F = [&](int v) { return draws_sum(n, sh.red, [&](long i) { return XI[i] <= v ? W[i] : 0.0; }); };
  const int vmax = (int)draws_max(n, sh.red, [&](long i) { return V[i] != -INFINITY ? (double)XI[i] : -INFINITY; });
  const int vmin = (int)-draws_max(n, sh.red, [&](long i) { return V[i] != -INFINITY ? -(double)XI[i] : -INFINITY; });
  for (int k = 0; k < 2; ++k) {
    int lo = vmin, hi = vmax;                              // v*: the smallest drawn value with F(v*) >= p, else the largest
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (F(mid) >= pr[k]) hi = mid; else lo = mid + 1; }
    const double vm = draws_max(n, sh.red, [&](long i) { return V[i] != -INFINITY && XI[i] < lo ? (double)XI[i] : -INFINITY; });
    q[k] = vm == -INFINITY ? (double)lo : loo_predict_interp(vm, (double)lo, F((int)vm), F(lo), pr[k]);
  }
  if (tid == 0) { o[0] = mean; o[1] = q[0]; o[2] = q[1]; o[3] = plt; o[4] = ple; o[5] = khat; }
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_predict_kernel);
static hipError_t loo_predict_cells(const LooPredictArgs& args, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  const long slice = loo_predict_slice(args.l.n);
  return cells_in_batches(args, slice, n_cells, scratch_bytes, scratch, [&](const LooPredictArgs& p, const CellLaunch& c) {
    return launch_cell_kernel(pick_kernel<ppcx_loo_predict_kernel_of>(c.lds, c.cols, p.l.lr != nullptr), p, c, p.l.sel_pad, slice, st);
  });
}

hipError_t loo_predict_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, uint32_t k0, double* out,
                                 size_t scratch_bytes, hipStream_t st) {
  return for_gene_batches(fc, kLooPredictFields, out, scratch_bytes, st,
                          [&](const LooArgs& a, const int* genes, int n_cells, DeviceBuffer<double>& scratch) {
    LooPredictArgs p;
    p.l = a; p.genes = genes; p.tc = tc; p.p_lo = p_lo; p.p_hi = p_hi; p.k0 = k0;
    return loo_predict_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

hipError_t loo_predict_columns(const GivenCells& gc, const int* x, const int* y, double p_lo, double p_hi, double* out,
                               size_t scratch_bytes, hipStream_t st) {
  const size_t n_cols = (size_t)gc.n_cols;
  DeviceBuffer<int> d_x, d_y;                            // outlive the walk, which drains the stream before it returns
  hipError_t e = d_x.upload(x, (size_t)gc.n * n_cols, st);
  if (e == hipSuccess) e = d_y.upload(y, n_cols, st);
  if (e != hipSuccess) return finish(e, st);
  return for_given_columns(gc, kLooPredictFields, out, st, [&](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    LooPredictArgs p;
    p.l = a; p.xcols = d_x.p; p.ycols = d_y.p; p.p_lo = p_lo; p.p_hi = p_hi;
    return loo_predict_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

}  // namespace ppcx
