// ppcx_loo_dev.h -- what the per-cell leave-one-out kernels share (ppcx_loo.hip: PSIS-LOO per cell; ppcx_loo_predict.hip: the
// leave-one-out predictive interval per cell; ppcx_reff.hip: the relative efficiency per cell). On the device: which cell a
// workgroup has and where its arrays live (cell_mem), the cell's linear predictor and log-likelihood from the transposed table,
// its ratios r = -ll (an ADVI fit: (log_p - log_g) - ll, ppcx_loo_ap.h), the fitted tail with the copies of the cutoff, a draw's
// log weight under the tie rule -- together the weights stage (loo_cell_verdict, loo_cell_weights) -- and the workgroup's sums
// for the exact sweeps of ppcx_ppc_exact.h (ExactBlockSums), the fill of (eta, ln phi) before them (loo_fill_eta_lnphi) and the
// plain exact predictive of a cell from the verdict to khat (loo_exact_cell).
// The table itself and a cell's read of it are ppcx_table.h's, shared with the posterior-predictive kernels.
// On the host: the one walk over a fit's cells in gene batches (for_gene_batches), its counterpart for host-given columns
// (for_given_columns) and the launch path: the batches of cells under the scratch bound (cells_in_batches), LDS against scratch
// (cell_launch), a kernel template's instantiation (pick_kernel) and its dynamic LDS (launch_cell_kernel); a statistic states its
// slice function, its kernel template and its argument block. The statistic is ppcx_loo.h; the workgroup pieces are ppcx_block.h
// and ppcx_psis_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_psis_dev.h"
#include "ppcx_loo.h"
#include "ppcx_loo_ap.h"
#include "ppcx_ppc_exact.h"
#include "ppcx_loo_exact.h"
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

// The workgroup's memory: the two selection arrays of sel_pad slots at the start of the dynamic LDS (K: the keys of the M + 1
// largest ratios, X: the tail's exceedances), then the cell's own arrays from V on, `slice` doubles: behind them in LDS, or in
// the workgroup's slice of the launch's scratch
struct CellMem { uint64_t* K; double* X; double* V; };
template <bool LDS>
__device__ __forceinline__ CellMem cell_mem(uint64_t* lds_u, const LooArgs& a, long slice) {
  double* X = reinterpret_cast<double*>(lds_u + a.sel_pad);
  return CellMem{lds_u, X, LDS ? X + a.sel_pad : a.scratch + (long)blockIdx.x * slice};
}

// The cell's ratios r = -ll into V[0 .. n); AP, the approximate-posterior statistic (ppcx_loo_ap.h step 0): r = a.lr - ll (an
// excluded cell: a.lr alone) and, where L is given, ll into L[0 .. n). Returns whether the cell is NaN (a NaN ratio, or +Inf
// where the cell is not excluded; AP: loo_ap_bad); otherwise N (the ratios that are not -Inf), the
// largest ratio and the largest ll. Every thread gets the same.
struct CellRatios { long N; double rmax, lmax; };
template <bool COLS, bool AP>
__device__ inline bool loo_cell_ratios(const LooArgs& a, const LooCell& c, bool excluded, double* V, double* L, PsisShared& sh,
                                       CellRatios* out) {
  const long n = a.n;
  bool bad = false; double cnt = 0.0, rmax = -INFINITY, lmax = -INFINITY;
  for (long i = threadIdx.x; i < n; i += kBlockThreads) {
    const double ll = COLS ? a.cols[(long)c.cell * n + i] : loo_cell_ll(a, c.gi, c.s, i, c.y);
    double r;
    if constexpr (AP) {
      const double lr = a.lr[i];
      r = loo_ap_ratio(lr, ll, excluded);
      bad = bad || loo_ap_bad(lr, ll, r, excluded);
    } else {
      r = -ll;
      bad = bad || isnan(r) || (!excluded && r == INFINITY);
    }
    if (r != -INFINITY) { cnt += 1.0; rmax = fmax(rmax, r); lmax = fmax(lmax, ll); }
    V[i] = r;
    if (AP && L) L[i] = ll;
  }
  bad = block_any(bad);
  if (bad) return true;
  out->N = (long)block_sum(cnt, sh.red);
  out->rmax = block_max(rmax, sh.red);
  out->lmax = block_max(lmax, sh.red);
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

// The log weight of every draw into W[0 .. n) from the ratios V (largest: mx) and their fitted tail; NORM: then the normalised
// weights exp(W - max) / sum in their place (a barrier is the caller's, before another thread's W is read)
template <bool NORM>
__device__ __forceinline__ void loo_cell_lw(const double* V, double* W, long n, double mx, const LooTail& lt, int M, const uint64_t* K,
                                            PsisShared& sh) {
  const int tid = threadIdx.x;
  if constexpr (!NORM) {
    for (long i = tid; i < n; i += kBlockThreads) W[i] = loo_draw_lw(V, i, mx, lt, M, K);
  } else {
    double mxw = -INFINITY;
    for (long i = tid; i < n; i += kBlockThreads) {
      const double lw = loo_draw_lw(V, i, mx, lt, M, K);
      W[i] = lw; mxw = fmax(mxw, lw);
    }
    mxw = block_max(mxw, sh.red);
    double sw = 0.0;
    for (long i = tid; i < n; i += kBlockThreads) { const double e = exp(W[i] - mxw); W[i] = e; sw += e; }
    sw = block_sum(sw, sh.red);
    for (long i = tid; i < n; i += kBlockThreads) W[i] = W[i] / sw;
  }
}

// The weights stage of a cell, once for the kernels that materialise weights (ppcx_loo_ap_kernel: log weights; ppcx_loo_predict_
// kernel, ppcx_loo_exact_kernel: normalised ones -- so their khat is the same bits by construction), in two steps:
// loo_cell_verdict: the ratios into m.V and what becomes of the cell. CELL_UNIFORM: a cell that a NUTS fit excludes is held out
// already -- the caller weights every draw alike and loo_cell_weights is not called.
// loo_cell_weights: the tail of psis_tail_len(N, r_eff) draws and the (log) weight of every draw into W; returns khat.
enum CellVerdict : int { CELL_NAN = 0, CELL_UNIFORM, CELL_WEIGHTED };
template <bool COLS, bool AP>
__device__ __forceinline__ CellVerdict loo_cell_verdict(const LooArgs& a, const LooCell& c, const CellMem& m, double* L, PsisShared& sh,
                                                        CellRatios* r) {
  if (loo_cell_ratios<COLS, AP>(a, c, c.excluded, m.V, L, sh, r)) return CELL_NAN;
  if (!AP && c.excluded) return CELL_UNIFORM;
  return r->N == 0 ? CELL_NAN : CELL_WEIGHTED;
}
template <bool NORM>
__device__ __forceinline__ double loo_cell_weights(const LooArgs& a, const LooCell& c, const CellMem& m, const CellRatios& r, double* W,
                                                   PsisShared& sh) {
  const int M = psis_tail_len(r.N, a.r_eff ? a.r_eff[c.cell] : 1.0);
  const LooTail lt = loo_cell_tail(m.V, a.n, r.N, M, m.K, m.X, a.sel_pad, sh);
  loo_cell_lw<NORM>(m.V, W, a.n, r.rmax, lt, M, m.K, sh);
  return lt.khat;
}

// The sums of ppc_exact_sweeps (ppcx_ppc_exact.h) by the workgroup over (eta_i, ln phi_i) = (E[i], LP[i]): a strided sweep and
// block_sum per sum, in the fixed order; every thread holds them. WEIGHTED: each term under W[i] (loo_exact_term)
template <bool WEIGHTED>
struct ExactBlockSums {
  const double* W; const double* E; const double* LP; long n; double* red;
  template <class F, int K>
  __device__ __forceinline__ void operator()(F f, double (&s)[K]) const {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (long i = threadIdx.x; i < n; i += kBlockThreads) {
      double t[K];
      (void)f(E[i], LP[i], t);
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += WEIGHTED ? loo_exact_term(W[i], t[k]) : t[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = block_sum(s[k], red);
  }
};

// (eta_i, ln phi_i) of every draw into E and LP, eta_i = src(i, &sigma_raw_i); returns whether a draw of the workgroup has
// invalid parameters (ppc_exact_invalid). Every thread gets the same.
template <class Src>
__device__ __forceinline__ bool loo_fill_eta_lnphi(long n, double log_tc, double* E, double* LP, Src src) {
  PPCX_NO_CONTRACT
  bool inval = false;
  for (long i = threadIdx.x; i < n; i += kBlockThreads) {
    double sg = 0.0;
    const double eta = src(i, &sg);
    const double lp = ppc_exact_lnphi(sg, log_tc);
    E[i] = eta; LP[i] = lp;
    inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
  }
  return block_any(inval);
}

// doubles per cell of the kernels that keep three arrays of n draws (ppcx_loo_exact_kernel and the moment-matched ones)
__host__ __device__ inline long loo_slice3(long n) { return 3 * n; }

// The exact predictive of cell c under plain PSIS weights (ppcx_loo_exact.h), from the verdict to khat: the ten fields into
// o[kLooExactFields]. m.V holds the ratios, then eta; behind it the log weights, then the weights, and ln phi (loo_slice3).
// ppcx_loo_exact_kernel is this function; the moment-matched kernels call it for a cell that was not matched, so their ten
// fields are ppcx_fit_loo_predict_exact's bits by construction. etacols / sgcols: the given columns' (COLS).
template <bool COLS, bool AP>
__device__ __forceinline__ void loo_exact_cell(const LooArgs& a, const LooCell& c, const CellMem& m, const double* etacols,
                                               const double* sgcols, double log_tc, double p_lo, double p_hi, double* o, PsisShared& sh) {
  PPCX_NO_CONTRACT
  const int tid = threadIdx.x;
  const long n = a.n;
  double* W = m.V + n;                                   // [n] log weights, then weights (m.V: [n] the ratios)
  double* LP = W + n;                                    // [n] ln phi
  double* E = m.V;                                       // [n] eta, once the ratios are dead
  // ---- the ratios, the tail, the normalised weight of every draw
  CellRatios cr;
  const CellVerdict verdict = loo_cell_verdict<COLS, AP>(a, c, m, nullptr, sh, &cr);
  if (verdict == CELL_NAN) { if (tid == 0) loo_exact_store_nan(o, c.y, c.excluded); return; }
  const bool uniform = verdict == CELL_UNIFORM;          // already held out: w_i = 1, every sum over n
  double khat = NAN;
  if (uniform) for (long i = tid; i < n; i += kBlockThreads) W[i] = 1.0;
  else khat = loo_cell_weights<true>(a, c, m, cr, W, sh);
  __syncthreads();                                       // no thread reads a ratio any more: V becomes E
  // ---- (eta, ln phi) of every draw
  const double* Tg = COLS ? nullptr : a.T + (long)c.gi * (a.C + 1) * n;
  const bool inval = loo_fill_eta_lnphi(n, log_tc, E, LP, [&](long i, double* sg) {
    const double eta = COLS ? etacols[(long)c.cell * n + i] : loo_cell_eta(a, Tg, c.s, i, sg);
    if (COLS) *sg = sgcols[(long)c.cell * n + i];
    return eta;
  });
  if (inval) { if (tid == 0) loo_exact_store_nan(o, c.y, c.excluded); return; }
  // ---- the moments, the two tails at y, the interval (ppc_exact_sweeps); khat beside its nine fields
  const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, c.y, c.excluded, uniform ? n : 1, p_lo, p_hi, tid == 0, o);
  if (tid == 0) o[kPpcExactFields] = ok ? khat : NAN;
}

// ---- the launch path (host)
// A launch over cells: whether a cell's arrays live in LDS (up to kPsisLdsDraws draws) or in the scratch, whether the cells
// are given columns, and how many there are. The one place that decides the first two.
struct CellLaunch { bool lds, cols; int n_blocks; };
inline CellLaunch cell_launch(const LooArgs& l, int n_blocks) { return CellLaunch{l.n <= kPsisLdsDraws, l.cols != nullptr, n_blocks}; }
// the LooArgs of a statistic's argument block (the block itself, or its member l)
inline LooArgs& cell_args(LooArgs& a) { return a; }
template <class P> auto cell_args(P& p) -> decltype((p.l)) { return p.l; }

// The instantiation of a kernel template for runtime flags, in the template's order: pick_kernel<KernelOf>(lds, cols, ..) where
// KernelOf::get<flags...>() names it (PPCX_KERNEL_OF(kernel) declares kernel_of so)
#define PPCX_KERNEL_OF(kernel) struct kernel##_of { template <bool... B> static constexpr auto get() { return &kernel<B...>; } }
template <class KernelOf, bool... B>
auto pick_kernel() { return KernelOf::template get<B...>(); }
template <class KernelOf, bool... B, class... Rest>
auto pick_kernel(bool flag, Rest... rest) {
  return flag ? pick_kernel<KernelOf, B..., true>(rest...) : pick_kernel<KernelOf, B..., false>(rest...);
}

// One workgroup of kBlockThreads per cell of the launch c, its dynamic LDS the two selection arrays (sel_pad slots each; 0:
// none) and, on the LDS path, the cell's `slice` doubles
template <class P>
hipError_t launch_cell_kernel(void (*kernel)(P), const P& p, const CellLaunch& c, int sel_pad, long slice, hipStream_t st) {
  const size_t bytes = sizeof(double) * (2 * (size_t)sel_pad + (c.lds ? (size_t)slice : 0));
  return launch_dynamic_lds(kernel, c.n_blocks, kBlockThreads, bytes, st, p);
}

// The cells of a statistic with argument block p (cell_args(p): its LooArgs) at `slice` doubles per cell, in batches: all at
// once where a cell's arrays live in LDS, else as many as the scratch bound holds. each(p, CellLaunch) launches the statistic's
// kernels over a batch, p's cell0 and scratch set. Asynchronous: `scratch` belongs to the caller, who synchronises before it goes.
template <class P, class Each>
hipError_t cells_in_batches(P p, long slice, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, Each each) {
  LooArgs& l = cell_args(p);
  hipError_t e = hipSuccess;
  int batch = n_cells;
  if (!cell_launch(l, 0).lds) {
    batch = column_batch(scratch_bytes, slice, n_cells);
    if (!scratch.p) e = scratch.alloc((size_t)slice * batch);
  }
  for (int c0 = 0; e == hipSuccess && c0 < n_cells; c0 += batch) {
    l.cell0 = c0; l.scratch = scratch.p;
    e = each(p, cell_launch(l, n_cells - c0 < batch ? n_cells - c0 : batch));
  }
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
// (device), its cells, the scratch) launches the statistic over cells_in_batches. The scratch is allocated by the first batch
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
