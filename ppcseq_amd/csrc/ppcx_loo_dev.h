// ppcx_loo_dev.h -- what the per-cell leave-one-out kernels share (ppcx_loo.hip: PSIS-LOO per cell; ppcx_loo_predict.hip: the
// leave-one-out predictive interval per cell; ppcx_reff.hip: the relative efficiency per cell). On the device: which cell a
// workgroup has, the cell's linear predictor and log-likelihood from the transposed table, its ratios r = -ll (an ADVI fit:
// (log_p - log_g) - ll, ppcx_loo_ap.h), the fitted tail with the copies of the cutoff, a draw's log weight under the tie rule.
// The table itself and a cell's read of it are ppcx_table.h's, shared with the posterior-predictive kernels.
// On the host: the one walk over a fit's cells in gene batches (for_gene_batches), its counterpart for host-given columns
// (for_given_columns) and the batches of cells under the scratch bound (loo_cell_batches); a statistic's drivers add their
// argument block and their kernel. The statistic is ppcx_loo.h; the workgroup pieces are ppcx_block.h and ppcx_psis_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_psis_dev.h"
#include "ppcx_loo.h"
#include "ppcx_loo_ap.h"
#include "ppcx_columns.h"
#include "ppcx_table.h"

namespace ppcx {

// The cell of this workgroup among the launch's cells: of the table's genes (gene gi of the table, sample s, its count y and
// whether the model holds it out) or of the given columns (their excluded flag; y = ycols[cell] where counts are given)
struct LooCell { int cell, gi, s, y; bool excluded; };
template <bool COLS>
__device__ __forceinline__ LooCell loo_cell(const LooArgs& a, const int* ycols = nullptr) {
  LooCell c{(int)(a.cell0 + blockIdx.x), 0, 0, 0, false};
  if (COLS) { c.excluded = a.excl && a.excl[c.cell] != 0; if (ycols) c.y = ycols[c.cell]; }
  else { const int ye = a.y[c.cell]; c.excluded = ye < 0; c.y = c.excluded ? -ye - 1 : ye; }
  c.gi = COLS ? 0 : c.cell / a.S; c.s = COLS ? 0 : c.cell - c.gi * a.S;
  return c;
}

// linear predictor of cell (gene gi of the table, sample s) at draw j, with sigma_raw where asked for: table_draw, as the
// posterior-predictive kernels read it
__device__ __forceinline__ double loo_cell_eta(const LooArgs& a, const double* Tg, int s, long j, double* sigma_raw = nullptr) {
  double eta, last;
  table_draw(Tg, a.n, a.C, a.expo[s], a.X, a.S, s, j, &eta, &last);
  if (sigma_raw) *sigma_raw = last;
  return eta;
}
// log-likelihood of cell (gene gi of the table, sample s) at draw j, count y >= 0
__device__ __forceinline__ double loo_cell_ll(const LooArgs& a, int gi, int s, long j, int y) {
  const double* Tg = a.T + (long)gi * (a.C + 1) * a.n;
  double sigma_raw;
  const double eta = loo_cell_eta(a, Tg, s, j, &sigma_raw);
  return loo_ll(y, eta, sigma_raw);
}

// The cell's ratios r = -ll into V[0 .. n). Returns whether the cell is NaN (a NaN ratio, or +Inf where the cell is not
// excluded); otherwise N (the ratios that are not -Inf), the largest ratio and the largest ll. Every thread gets the same.
template <bool COLS>
__device__ inline bool loo_cell_ratios(const LooArgs& a, int cell, int gi, int s, int y, bool excluded, double* V, PsisShared& sh,
                                       long* N, double* rmax_out, double* lmax_out) {
  const int tid = threadIdx.x;
  const long n = a.n;
  bool bad = false; double cnt = 0.0, rmax = -INFINITY, lmax = -INFINITY;
  for (long i = tid; i < n; i += kBlockThreads) {
    const double ll = COLS ? a.cols[(long)cell * n + i] : loo_cell_ll(a, gi, s, i, y);
    const double r = -ll;
    bad = bad || isnan(r) || (!excluded && r == INFINITY);
    if (r != -INFINITY) { cnt += 1.0; rmax = fmax(rmax, r); lmax = fmax(lmax, ll); }
    V[i] = r;
  }
  bad = block_any(bad);
  if (bad) return true;
  *N = (long)block_sum(cnt, sh.red);
  *rmax_out = block_max(rmax, sh.red);
  *lmax_out = block_max(lmax, sh.red);
  return false;
}

// The same for the approximate-posterior statistic (ppcx_loo_ap.h step 0): r = a.lr - ll (an excluded cell: a.lr alone) into
// V[0 .. n) and, where L is given, ll into L[0 .. n). Also NaN: a cell without a participating draw.
template <bool COLS>
__device__ inline bool loo_ap_cell_ratios(const LooArgs& a, int cell, int gi, int s, int y, bool excluded, double* V, double* L,
                                          PsisShared& sh, long* N, double* rmax_out, double* lmax_out) {
  const int tid = threadIdx.x;
  const long n = a.n;
  bool bad = false; double cnt = 0.0, rmax = -INFINITY, lmax = -INFINITY;
  for (long i = tid; i < n; i += kBlockThreads) {
    const double ll = COLS ? a.cols[(long)cell * n + i] : loo_cell_ll(a, gi, s, i, y);
    const double lr = a.lr[i];
    const double r = loo_ap_ratio(lr, ll, excluded);
    bad = bad || loo_ap_bad(lr, ll, r, excluded);
    if (r != -INFINITY) { cnt += 1.0; rmax = fmax(rmax, r); lmax = fmax(lmax, ll); }
    V[i] = r;
    if (L) L[i] = ll;
  }
  bad = block_any(bad);
  if (bad) return true;
  *N = (long)block_sum(cnt, sh.red);
  *rmax_out = block_max(rmax, sh.red);
  *lmax_out = block_max(lmax, sh.red);
  return *N == 0;
}

// The tail of the ratios V (ppcx_loo.h step 2): k-hat, sigma, whether the tail is smoothed, and where it is, n_eq = the copies
// of the cutoff among all the draws (tl.want of them are among the M + 1 largest, one of those the cutoff itself).
struct LooTail { double khat = INFINITY, sigma = 0.0; bool smooth = false; int n_eq = 0; PsisTail tl{}; };
__device__ inline LooTail loo_cell_tail(const double* V, long n, long N, int M, uint64_t* K, double* X, int sel_pad, PsisShared& sh) {
  LooTail t;
  if (psis_tail(V, n, N, M, K, X, sel_pad, sh, &t.tl) == PSIS_TAIL_FITTED) {
    t.khat = psis_adjust(t.tl.k_mean, M);
    t.sigma = -t.tl.k_mean / t.tl.theta_hat;
    t.smooth = loo_smooth_ok(t.khat, t.sigma);
    if (t.smooth) {
      double eq = 0.0;
      for (long i = threadIdx.x; i < n; i += kBlockThreads) eq += psis_key(V[i]) == t.tl.key ? 1.0 : 0.0;
      t.n_eq = (int)block_sum(eq, sh.red);
    }
  }
  return t;
}

// The log weight of draw i (ppcx_loo_predict.h step 2) from the ratios V, their fitted tail and the sorted keys K[0 .. M]: the
// tail position of a draw by binary search, and for a key that occurs more than once among the M + 1 largest a scan of the
// earlier draws (ties are rare)
__device__ __forceinline__ int loo_draw_tail_pos(const double* V, long i, double r, const LooTail& lt, int M, const uint64_t* K) {
  if (!lt.smooth || r == -INFINITY) return 0;
  const PsisTail& tl = lt.tl;
  const uint64_t k = psis_key(r);
  if (k < tl.key) return 0;
  const bool scan = k == tl.key ? tl.want > 1 : loo_predict_tied(K, M, loo_predict_lower_bound(K, M, k));
  long before = 0;
  if (scan) for (long i2 = 0; i2 < i; ++i2) before += psis_key(V[i2]) == k ? 1 : 0;
  return loo_predict_tail_pos(k, K, M, tl.key, tl.want, lt.n_eq, before);
}
__device__ __forceinline__ double loo_draw_lw(const double* V, long i, double mx, const LooTail& lt, int M, const uint64_t* K) {
  const double r = V[i];
  return loo_predict_lw(r, mx, loo_draw_tail_pos(V, i, r, lt, M, K), M, lt.khat, lt.sigma, lt.tl.ec);
}

// Cells of a launch in batches: all at once where a cell's arrays live in LDS (slice = 0), else as many as the scratch bound
// holds at `slice` doubles per cell. launch(first cell, cells, scratch). Asynchronous: `scratch` belongs to the caller, who
// synchronises before it goes.
template <class Launch>
hipError_t loo_cell_batches(int n_cells, long slice, size_t scratch_bytes, DeviceBuffer<double>& scratch, Launch launch) {
  hipError_t e = hipSuccess;
  int batch = n_cells;
  if (slice > 0) {
    batch = column_batch(scratch_bytes, slice, n_cells);
    if (!scratch.p) e = scratch.alloc((size_t)slice * batch);
  }
  for (int c0 = 0; e == hipSuccess && c0 < n_cells; c0 += batch)
    e = launch(c0, n_cells - c0 < batch ? n_cells - c0 : batch, scratch.p);
  return e;
}

// What a walk over a fit's cells keeps on the device for all of its batches: the gene ids, the encoded counts and r_eff
// (where given), and from them the LooArgs of genes g0 .. g0 + ng of a table T that holds those genes from its start.
struct FitCellsDev {
  DeviceBuffer<int> genes, y; DeviceBuffer<double> r_eff;
  hipError_t upload(const FitCells& fc, hipStream_t st) {
    const size_t ncells = (size_t)fc.n_genes * fc.d.S;
    hipError_t e = genes.upload(fc.genes, (size_t)fc.n_genes, st);
    if (e == hipSuccess) e = y.upload(fc.yenc, ncells, st);
    if (e == hipSuccess && fc.r_eff) e = r_eff.upload(fc.r_eff, ncells, st);
    return e;
  }
  LooArgs args(const FitCells& fc, const double* T, int g0, int ng) const {
    const size_t c0 = (size_t)g0 * fc.d.S;
    LooArgs a;
    a.T = T; a.y = y.p + c0; a.expo = fc.expo; a.X = fc.X; a.S = fc.d.S; a.C = fc.d.C; a.n = fc.n;
    a.r_eff = r_eff.p ? r_eff.p + c0 : nullptr; a.lr = fc.log_ratio;
    a.n_cells = ng * fc.d.S; a.sel_pad = loo_sel_pad(fc.n, fc.r_eff_min);
    return a;
  }
};

// The cells of a fit in batches of column_batch(scratch_bytes, ..) genes: each batch's transposed table T (never the table of
// all the genes), then body(the batch's LooArgs with `out` at its part of the device output [cells][fields], its gene ids
// (device), its cells, the scratch) launches the statistic over loo_cell_batches. The scratch is allocated by the first batch
// that needs it and serves the later ones; every buffer lives until the stream has drained. The output is copied to out (host)
// at the end. Synchronous.
template <class Body>
hipError_t for_gene_batches(const FitCells& fc, int fields, double* out, size_t scratch_bytes, hipStream_t st, Body body) {
  const int S = fc.d.S, ncol = fc.d.C + 1;
  const size_t ncells = (size_t)fc.n_genes * S;
  const int gb = column_batch(scratch_bytes, (long)ncol * fc.n, fc.n_genes);
  FitCellsDev dev; DeviceBuffer<double> d_T, d_out, d_scr;
  hipError_t e = dev.upload(fc, st);
  if (e == hipSuccess) e = d_out.alloc((size_t)fields * ncells);
  if (e == hipSuccess) e = d_T.alloc((size_t)ncol * (size_t)fc.n * gb);
  for (int g0 = 0; e == hipSuccess && g0 < fc.n_genes; g0 += gb) {
    const int ng = fc.n_genes - g0 < gb ? fc.n_genes - g0 : gb;
    e = launch_loo_table_kernel(fc.draws, fc.n, fc.d, dev.genes.p + g0, ng, d_T.p, st);
    if (e != hipSuccess) break;
    LooArgs a = dev.args(fc, d_T.p, g0, ng);
    a.out = d_out.p + (size_t)g0 * S * fields;
    e = body(a, dev.genes.p + g0, ng * S, d_scr);
  }
  if (e == hipSuccess) e = d_out.download(out, (size_t)fields * ncells, st);
  return finish(e, st);
}

// The same for host-given columns (testing build): body(the LooArgs of all the columns, null, n_cols, the scratch).
template <class Body>
hipError_t for_given_columns(const GivenCells& gc, int fields, double* out, hipStream_t st, Body body) {
  const size_t n_cols = (size_t)gc.n_cols;
  DeviceBuffer<double> d_cols, d_reff, d_lr, d_out, d_scr; DeviceBuffer<int> d_excl;
  hipError_t e = d_cols.upload(gc.cols, (size_t)gc.n * n_cols, st);
  if (e == hipSuccess && gc.excl) e = d_excl.upload(gc.excl, n_cols, st);
  if (e == hipSuccess && gc.r_eff) e = d_reff.upload(gc.r_eff, n_cols, st);
  if (e == hipSuccess && gc.log_ratio) e = d_lr.upload(gc.log_ratio, (size_t)gc.n, st);
  if (e == hipSuccess) e = d_out.alloc((size_t)fields * n_cols);
  if (e == hipSuccess) {
    LooArgs a;
    a.cols = d_cols.p; a.excl = d_excl.p; a.r_eff = d_reff.p; a.lr = d_lr.p; a.n = gc.n; a.n_cells = gc.n_cols; a.out = d_out.p;
    a.sel_pad = loo_sel_pad(gc.n, gc.r_eff_min);
    e = body(a, (const int*)nullptr, gc.n_cols, d_scr);
  }
  if (e == hipSuccess) e = d_out.download(out, (size_t)fields * n_cols, st);
  return finish(e, st);
}

}  // namespace ppcx
