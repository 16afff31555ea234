// ppcx_loo_dev.h -- what the two leave-one-out kernels share on the device (ppcx_loo.hip: PSIS-LOO per cell; ppcx_loo_predict.hip:
// the leave-one-out predictive interval per cell) and in their drivers: the cell's linear predictor and log-likelihood from the
// transposed table, its ratios r = -ll, the fitted tail with the copies of the cutoff, and the batches of cells under the scratch
// bound. The statistic is ppcx_loo.h; the workgroup pieces are ppcx_block.h and ppcx_psis_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_psis_dev.h"
#include "ppcx_loo.h"
#include "ppcx_columns.h"

namespace ppcx {

// linear predictor of cell (gene gi of the table, sample s) at draw j: the expression of the posterior-predictive kernels
__device__ __forceinline__ double loo_cell_eta(const LooArgs& a, const double* Tg, int s, long j) {
  double eta = a.expo[s] + a.X[s] * Tg[j];
  for (int cc = 1; cc < a.C; ++cc) eta += a.X[(long)cc * a.S + s] * Tg[(long)cc * a.n + j];
  return eta;
}
// log-likelihood of cell (gene gi of the table, sample s) at draw j, count y >= 0
__device__ __forceinline__ double loo_cell_ll(const LooArgs& a, int gi, int s, long j, int y) {
  const double* Tg = a.T + (long)gi * (a.C + 1) * a.n;
  return loo_ll(y, loo_cell_eta(a, Tg, s, j), Tg[(long)a.C * a.n + j]);
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

}  // namespace ppcx
