// ppcx_loo_exact.hip -- gfx950 kernel of the exact leave-one-out predictive tail probabilities and interval per cell
// (ppcx_fit_loo_predict_exact, ppcx_fit_loo_predict_exact_approx, include/ppcx.h; the statistic: ppcx_loo_exact.h, the weights:
// ppcx_loo_dev.h, the negative-binomial tails: ppcx_nbcdf.h). The walk over the cells is ppcx_loo_dev.h's (for_gene_batches,
// for_given_columns); the drivers at the end of this file add the argument block and the kernel.
//
//   ppcx_loo_exact_kernel  one workgroup of kBlockThreads per cell, a sibling of ppcx_loo_predict_kernel (the weights) and of
//                          ppcx_ppc_exact_kernel (everything after them). The cell's ratios from the transposed table T
//                          (ppcx_loo_table_kernel) or the given columns by loo_cell_ratios / loo_ap_cell_ratios, the tail by
//                          loo_cell_tail, the log weight of every draw by loo_draw_lw, the normalised weights: the calls and the
//                          order of ppcx_loo_predict_kernel, so khat is its khat bit for bit. The ratios are dead once the
//                          weights exist; only then (eta_i, ln phi_i) of every draw are formed, eta into the ratios' place. (The
//                          table is therefore read twice per draw, as ppcx_loo_predict_kernel reads it for its counts: one
//                          read would need the ratios' loop restated here instead of called.) Every later sweep reads
//                          (w_i, eta_i, ln phi_i) strided and reduces with block_sum in the fixed order: the mean, the two
//                          variance sums, the two tails at y, and one sweep (two sums) per step of each quantile search,
//                          whose control flow is uniform because every thread holds the same sums.
//                          A cell that a NUTS fit excludes runs the same sweeps with w_i = 1 and every sum divided by n
//                          (ppcx_loo_exact.h step 5): ppcx_ppc_exact_kernel's bits.
//                          AP: the ratios of an ADVI fit, (log_p - log_g) - ll; an excluded cell weighted by log_p - log_g.
//                          Per draw 24 bytes in three arrays -- ratio then eta (8), log weight then weight (8), ln phi (8) --
//                          in LDS up to kPsisLdsDraws draws, beside the two selection arrays (16 bytes per slot of
//                          loo_sel_pad: 4 KB at 4 096 draws and r_eff = 1), in the workgroup's slice of a bounded global scratch
//                          beyond. At 4 096 draws that is 96 KB + 4 KB + 2.8 KB static: ONE workgroup per CU of 160 KB, as
//                          four arrays (128 KB) would give; the third array's saving shows below 3 100 draws, where two
//                          workgroups fit (four arrays: below 2 300), three below 2 000; a fit of 1 000 draws takes 26 KB and
//                          the registers bind first (146 VGPRs: three workgroups per CU). The layout was
//                          chosen on this arithmetic alone: the kernel has NOT been timed, against the four-array form or at
//                          all.
// Every reduction runs in a fixed order and a cell reads nothing of another cell: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_dev.h"
#include "ppcx_loo_exact.h"

namespace ppcx {

struct LooExactArgs {
  LooArgs l;                       // the table or the ll columns (l.cols), y, r_eff, lr, n, the cells, sel_pad (l.scratch unused)
  const double* etacols = nullptr; // [cells][n] linear predictors of the given columns (testing build)
  const double* sgcols = nullptr;  // [cells][n] sigma_raw of the given columns
  const int* ycols = nullptr;      // [cells] observed counts of the given columns
  double log_tc = 0.0, p_lo = 0.025, p_hi = 0.975;
  double* scratch = nullptr; long slice = 0;   // [launch's cells][slice] doubles: the long path's three arrays
  double* out = nullptr;           // [cells][kLooExactFields] (= l.out)
};

// doubles of scratch per cell on the long path: ratio / eta [n], log weight / weight [n], ln phi [n]
static long loo_exact_slice(long n) { return 3 * n; }

// AP: the weights of an ADVI fit (ppcx_loo_ap.h)
template <bool LDS, bool COLS, bool AP>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_exact_kernel(LooExactArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  const LooArgs& a = p.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  uint64_t* K = lds_u;                                   // [sel_pad] keys of the M + 1 largest ratios
  double* X = reinterpret_cast<double*>(lds_u + a.sel_pad);            // [sel_pad] the tail's exceedances
  double* V = LDS ? X + a.sel_pad : p.scratch + (long)blockIdx.x * p.slice;   // [n] the ratios; then E: eta
  double* W = V + n;                                     // [n] log weights, then weights
  double* LP = W + n;                                    // [n] ln phi
  double* E = V;
  const LooCell c = loo_cell<COLS>(a, p.ycols);
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  const bool excluded = c.excluded;
  double* o = p.out + (long)cell * kLooExactFields;
  auto all_nan = [&]() { if (tid == 0) loo_exact_store_nan(o, y, excluded); };
  // ---- the ratios
  long N; double rmax, lmax;
  if constexpr (AP) {
    if (loo_ap_cell_ratios<COLS>(a, cell, gi, s, y, excluded, V, nullptr, sh, &N, &rmax, &lmax)) { all_nan(); return; }
  } else {
    if (loo_cell_ratios<COLS>(a, cell, gi, s, y, excluded, V, sh, &N, &rmax, &lmax)) { all_nan(); return; }
  }
  const bool uniform = !AP && excluded;                  // already held out: w_i = 1, every sum over n
  if (!uniform && N == 0) { all_nan(); return; }
  const long den = uniform ? n : 1;
  double khat = NAN;
  if (uniform) {
    for (long i = tid; i < n; i += kBlockThreads) W[i] = 1.0;
  } else {
    // ---- the tail, the log weight of every draw, the normalised weights
    const int M = psis_tail_len(N, a.r_eff ? a.r_eff[cell] : 1.0);
    const LooTail lt = loo_cell_tail(V, n, N, M, K, X, a.sel_pad, sh);
    double mxw = -INFINITY;
    for (long i = tid; i < n; i += kBlockThreads) {
      const double lw = loo_draw_lw(V, i, rmax, lt, M, K);
      W[i] = lw; mxw = fmax(mxw, lw);
    }
    mxw = block_max(mxw, sh.red);
    double sw = 0.0;
    for (long i = tid; i < n; i += kBlockThreads) { const double e = exp(W[i] - mxw); W[i] = e; sw += e; }
    sw = block_sum(sw, sh.red);
    for (long i = tid; i < n; i += kBlockThreads) W[i] = W[i] / sw;
    khat = lt.khat;
  }
  __syncthreads();                                       // no thread reads a ratio any more: V becomes E
  // ---- (eta, ln phi) of every draw
  bool inval = false;
  {
    const double* Tg = COLS ? nullptr : a.T + (long)gi * (a.C + 1) * n;
    for (long i = tid; i < n; i += kBlockThreads) {
      double sg = 0.0;
      const double eta = COLS ? p.etacols[(long)cell * n + i] : loo_cell_eta(a, Tg, s, i, &sg);
      if (COLS) sg = p.sgcols[(long)cell * n + i];
      const double lp = ppc_exact_lnphi(sg, p.log_tc);
      E[i] = eta; LP[i] = lp;
      inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
    }
  }
  if (block_any(inval)) { all_nan(); return; }
  // ---- the moments
  double sm = 0.0;
  for (long i = tid; i < n; i += kBlockThreads) sm += loo_exact_term(W[i], exp(E[i]));
  const double mean = block_sum(sm, sh.red) / (double)den;
  double ev = 0.0, dv = 0.0;
  for (long i = tid; i < n; i += kBlockThreads) {
    double e1, d1;
    ppc_exact_var_terms(E[i], ppc_exact_phi(LP[i]), mean, &e1, &d1);
    ev += loo_exact_term(W[i], e1); dv += loo_exact_term(W[i], d1);
  }
  ev = block_sum(ev, sh.red);
  dv = block_sum(dv, sh.red);
  const double sd = ppc_exact_sd(ev, dv, den);
  // ---- the two tails at y
  double sle = 0.0, sge = 0.0;
  for (long i = tid; i < n; i += kBlockThreads) {
    double t0, t1;
    const double lp = LP[i];
    (void)nb2_log_tails_ln(y, E[i], ppc_exact_phi(lp), lp, &t0, &t1);
    sle += loo_exact_term(W[i], t0); sge += loo_exact_term(W[i], t1);
  }
  sle = block_sum(sle, sh.red);
  sge = block_sum(sge, sh.red);
  // ---- the interval: every F is one sweep, every thread holds its value
  auto F = [&](int k) {
    double L = 0.0, U = 0.0;
    for (long i = tid; i < n; i += kBlockThreads) {
      double le, gt, pm; int it;
      const double lp = LP[i];
      nb2_cdf_pair(k, E[i], ppc_exact_phi(lp), lp, &le, &gt, &pm, &it);
      L += loo_exact_term(W[i], le); U += loo_exact_term(W[i], gt);
    }
    L = block_sum(L, sh.red);
    U = block_sum(U, sh.red);
    return ppc_exact_F(L, U, den);
  };
  int c0, w0;
  ppc_exact_bracket(mean, sd, &c0, &w0);
  const int lower = ppc_exact_quantile(p.p_lo, c0, w0, F);
  const int upper = ppc_exact_quantile(p.p_hi, c0, w0, F);
  if (tid == 0) {
    if (isnan(sle) || isnan(sge) || lower < 0 || upper < 0) loo_exact_store_nan(o, y, excluded);
    else loo_exact_store(o, mean, sd, sle / (double)den, sge / (double)den, lower, upper, y, excluded, khat);
  }
}

// ---- launch helpers (host)
static hipError_t launch_loo_exact_kernel(const LooExactArgs& p, int n_blocks, hipStream_t st) {
  const bool lds = p.l.n <= kPsisLdsDraws, cols = p.l.cols != nullptr;
  const size_t bytes = sizeof(double) * (2 * (size_t)p.l.sel_pad + (lds ? (size_t)loo_exact_slice(p.l.n) : 0));
  void (*kernel)(LooExactArgs);
  if (p.l.lr) kernel = lds ? (cols ? ppcx_loo_exact_kernel<true, true, true> : ppcx_loo_exact_kernel<true, false, true>)
                           : (cols ? ppcx_loo_exact_kernel<false, true, true> : ppcx_loo_exact_kernel<false, false, true>);
  else kernel = lds ? (cols ? ppcx_loo_exact_kernel<true, true, false> : ppcx_loo_exact_kernel<true, false, false>)
                    : (cols ? ppcx_loo_exact_kernel<false, true, false> : ppcx_loo_exact_kernel<false, false, false>);
  return launch_dynamic_lds(kernel, n_blocks, kBlockThreads, bytes, st, p);
}
static hipError_t loo_exact_cells(LooExactArgs p, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  p.slice = p.l.n > kPsisLdsDraws ? loo_exact_slice(p.l.n) : 0;
  return loo_cell_batches(n_cells, p.slice, scratch_bytes, scratch, [&](int c0, int nc, double* scr) {
    p.l.cell0 = c0; p.scratch = scr;
    return launch_loo_exact_kernel(p, nc, st);
  });
}

// a NUTS fit (fc.log_ratio null) or an ADVI fit (fc.log_ratio: log_p - log_g of the draws)
hipError_t loo_exact_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, double* out, size_t scratch_bytes,
                               hipStream_t st) {
  const double log_tc = log(tc);
  return for_gene_batches(fc, kLooExactFields, out, scratch_bytes, st,
                          [&](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    LooExactArgs p;
    p.l = a; p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi; p.out = a.out;
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
    p.l = a; p.etacols = d_eta.p; p.sgcols = d_sg.p; p.ycols = d_y.p; p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi; p.out = a.out;
    return loo_exact_cells(p, n_cells, scratch_bytes, scratch, st);
  });
}

}  // namespace ppcx
