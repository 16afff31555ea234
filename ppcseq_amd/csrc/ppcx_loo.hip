// ppcx_loo.hip -- gfx950 kernels of PSIS-LOO per observed cell (ppcx_fit_loo, ppcx_fit_get_log_lik, include/ppcx.h; the
// statistic: ppcx_loo.h). The walk over a fit's cells in gene batches is ppcx_loo_dev.h's (for_gene_batches); the drivers at
// the end of this file add the kernel to it.
//
//   ppcx_loo_table_kernel  the per-draw parameters of the requested genes, transposed: T[g][c][draw], c = 0 intercept,
//                          1 .. C - 1 slopes (0 for a gene without slopes), C sigma_raw: the table of ppcx_table.h (table_tiles,
//                          which ppcx_ppc_table_kernel of ppcx_ppc.hip runs too) for a gene list, the last row left as it is.
//   ppcx_loo_ll_kernel     the log-likelihood matrix itself, [draw][cell] (ppcx_fit_get_log_lik): one thread per (draw, cell).
//   ppcx_loo_kernel        one workgroup per cell: the cell's n log-likelihoods from T (the S cells of a gene read the same rows
//                          of T, through L2), as ratios r = -ll in LDS (up to kPsisLdsDraws draws) or in the workgroup's slice
//                          of a bounded global scratch; the M + 1 largest selected exactly and sorted (ppcx_psis_dev.h, the
//                          radix selection of the Pareto-k kernel), the profile fit, the smoothed tail and three logsumexp
//                          reductions (lpd; the weights; the weights times the likelihood). With MCSE (ppcx_fit_loo_mcse) one
//                          more sweep over the same terms with the known normaliser gives sum w^2 and sum w^2 expm1^2, then
//                          the 1000 Blom scores, at most four per thread in registers, the Monte-Carlo standard error. The
//                          testing build runs it on host-given columns too.
//   ppcx_loo_ap_kernel     the same for an ADVI fit (ppcx_fit_loo_approx; ppcx_loo_ap.h): the ratios r = (log_p - log_g) - ll no
//                          longer determine ll, so a draw keeps r, ll and its log weight lw -- 24 bytes, in LDS up to
//                          kPsisLdsDraws draws (96 KB beside the two selection arrays), in the workgroup's slice of the scratch
//                          beyond. lw of a draw as in the predictive kernel (loo_draw_lw: binary search in the sorted tail keys,
//                          a scan of the earlier draws only for keys that occur more than once), written once; the logsumexps
//                          then run over the draws in the fixed strided order. An excluded cell takes the same path with
//                          r = log_p - log_g.
// Every reduction runs in a fixed order and a cell reads nothing of another cell: its fields are the same bits whatever else is
// requested and however the work is batched. The G S x n matrix is never materialised for LOO.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "ppcx_loo_dev.h"

namespace ppcx {

__global__ __launch_bounds__(256) void ppcx_loo_table_kernel(const double* draws, long n_draws, Dims d, const int* genes,
                                                             int n_genes, double* T) {
  table_tiles<false>(draws, n_draws, d, genes, n_genes, 1.0, T);
}

__global__ __launch_bounds__(256) void ppcx_loo_ll_kernel(LooArgs a, long j0, long n_rows, double* out) {
  const long n_cells = (long)a.n_cells;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_rows * n_cells) return;
  const long jr = t / n_cells;
  const int cell = (int)(t - jr * n_cells);
  const int gi = cell / a.S, s = cell - gi * a.S;
  const int ye = a.y[cell];
  out[t] = loo_cell_ll(a, gi, s, j0 + jr, ye < 0 ? -ye - 1 : ye);
}

// doubles per cell of the approximate-posterior kernel: r [n], ll [n], lw [n]
__host__ __device__ inline long loo_ap_slice(long n) { return 3 * n; }

struct LooTerms { double a, b; };                // running max or sum of the two logsumexps: a over lw + ll, b over lw
enum LooSweep : int { LOO_MAX = 0, LOO_SUM, LOO_MCSE };   // what a sweep over the terms accumulates

// ppcx_loo.h steps 7 - 8 by the workgroup: the scores in registers, mean and variance by fixed-order block sums
__device__ inline double loo_mcse_blom(double c, double r_eff, double* red) {
  PPCX_NO_CONTRACT
  constexpr int kPer = (kLooMcseScores + kBlockThreads - 1) / kBlockThreads;
  double x[kPer];
  double s = 0.0, cnt = 0.0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int j = q * kBlockThreads + (int)threadIdx.x + 1;
    x[q] = j <= kLooMcseScores ? loo_mcse_score(j, c) : NAN;
    if (!isnan(x[q])) { s += x[q]; cnt += 1.0; }
  }
  s = block_sum(s, red);
  cnt = block_sum(cnt, red);
  const double mean = s / cnt;
  double ss = 0.0;
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (!isnan(x[q])) { const double d = x[q] - mean; ss += d * d; }
  ss = block_sum(ss, red);
  return loo_mcse_from(ss, cnt, r_eff);
}

template <bool LDS, bool COLS, bool MCSE>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_kernel(LooArgs a) {
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  const int tid = threadIdx.x;
  const long n = a.n;
  const CellMem m = cell_mem<LDS>(lds_u, a, n);
  uint64_t* K = m.K; double* X = m.X;
  double* V = m.V;                                       // [n] the cell's ratios r = -ll
  const LooCell c = loo_cell<COLS>(a);                   // of this launch's cells (the table's genes, or the given columns)
  const int cell = c.cell;
  const bool excluded = c.excluded;
  double* o = a.out + (long)cell * (MCSE ? kLooMcseFields : kLooFields);
  // ---- the ratios; NaN / +Inf; N (the -Inf ratios take no part); the largest ratio and the largest ll
  CellRatios cr;
  if (loo_cell_ratios<COLS, false>(a, c, excluded, V, nullptr, sh, &cr)) {
    if (tid == 0) {
      o[0] = o[1] = o[2] = o[3] = NAN;
      if constexpr (MCSE) o[4] = o[5] = NAN;
    }
    return;
  }
  const long N = cr.N; const double rmax = cr.rmax, lmax = cr.lmax;
  // ---- lpd = logsumexp(ll) - log N
  const double sl = draws_sum(n, sh.red, [&](long i) { const double r = V[i]; return r != -INFINITY ? exp(-r - lmax) : 0.0; });
  const double lpd = N > 0 ? (lmax == -INFINITY ? -INFINITY : lmax + log(sl)) - log((double)N) : NAN;
  if (excluded) {                                        // already held out: the exact held-out predictive density
    if (tid == 0) { o[0] = lpd; o[1] = 0.0; o[2] = -2.0 * lpd; o[3] = NAN; }
    if constexpr (MCSE) {                                // uniform weights 1 / N
      const double e = loo_mcse_frame(lpd, -rmax, lmax), re = a.r_eff ? a.r_eff[cell] : 1.0;
      const double sd = draws_sum(n, sh.red, [&](long i) { const double r = V[i]; return r != -INFINITY ? loo_mcse_uniform_term(-r, e) : 0.0; });
      const double mc = N > 0 ? loo_mcse_blom(sqrt(loo_mcse_uniform_c2(sd, N)), re, sh.red) : NAN;
      if (tid == 0) { o[4] = mc; o[5] = N > 0 ? (double)N * re : NAN; }
    }
    return;
  }
  // ---- the tail: M + 1 largest, the profile fit, k-hat and sigma
  const double mx = rmax;                                // the tail's own mx is this value (it exists only where M >= 5)
  const int M = psis_tail_len(N, a.r_eff ? a.r_eff[cell] : 1.0);
  const LooTail lt = loo_cell_tail(V, n, N, M, K, X, a.sel_pad, sh);
  const double khat = lt.khat, sigma = lt.sigma;
  const bool smooth = lt.smooth;
  const PsisTail& tl = lt.tl;
  const int n_extra = smooth ? lt.n_eq - (tl.want - 1) : 0;   // copies of the cutoff outside the tail: all of them but want - 1
  // ---- logsumexp(lw + ll) and logsumexp(lw): a raw draw has lw = r - mx (<= 0), a tail draw the smoothed value truncated at 0
  // (an MCSE sweep: mxv = {e, logsumexp(lw)}, a the sum of w^2 and b that of w^2 expm1(ll - e)^2)
  auto terms = [&](LooSweep sweep, LooTerms mxv) {
    const bool sum = sweep != LOO_MAX;
    LooTerms t{sum ? 0.0 : -INFINITY, sum ? 0.0 : -INFINITY};
    auto add = [&](double lw, double r, double mult) {
      if constexpr (MCSE) if (sweep == LOO_MCSE) { loo_mcse_add(lw, -r, mxv.b, mxv.a, mult, &t.a, &t.b); return; }
      const double va = lw - r;
      if (sum) { t.a += mult * exp(va - mxv.a); t.b += mult * exp(lw - mxv.b); }
      else { t.a = fmax(t.a, va); t.b = fmax(t.b, lw); }
    };
    for (long i = tid; i < n; i += kBlockThreads) {
      const double r = V[i];
      if (r == -INFINITY || (smooth && psis_key(r) >= tl.key)) continue;
      add(r - mx, r, 1.0);
    }
    if (smooth) {
      for (int j = tid; j < M; j += kBlockThreads) {
        const double sm = loo_smoothed(j + 1, M, khat, sigma, tl.ec);
        add(sm > 0.0 ? 0.0 : sm, psis_unkey(K[j + 1]), 1.0);
      }
      if (tid == 0 && n_extra > 0) { const double c = tl.cut; add(c - mx, c, (double)n_extra); }
    }
    return t;
  };
  LooTerms m0 = terms(LOO_MAX, LooTerms{0.0, 0.0});
  m0.a = block_max(m0.a, sh.red);
  m0.b = block_max(m0.b, sh.red);
  LooTerms s0 = terms(LOO_SUM, m0);
  s0.a = block_sum(s0.a, sh.red);
  s0.b = block_sum(s0.b, sh.red);
  const double elpd = (m0.a + log(s0.a)) - (m0.b + log(s0.b));
  if (tid == 0) { o[0] = elpd; o[1] = lpd - elpd; o[2] = -2.0 * elpd; o[3] = khat; }
  if constexpr (MCSE) {
    const double re = a.r_eff ? a.r_eff[cell] : 1.0;
    LooTerms q = terms(LOO_MCSE, LooTerms{loo_mcse_frame(elpd, -rmax, lmax), m0.b + log(s0.b)});
    q.a = block_sum(q.a, sh.red);
    q.b = block_sum(q.b, sh.red);
    const double mc = loo_mcse_blom(sqrt(q.b), re, sh.red);
    if (tid == 0) { o[4] = mc; o[5] = re / q.a; }
  }
}

template <bool LDS, bool COLS>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_ap_kernel(LooArgs a) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  const int tid = threadIdx.x;
  const long n = a.n;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_ap_slice(n));
  const double* V = m.V;                                 // [n] the ratios
  double* L = m.V + n;                                   // [n] the log-likelihoods
  double* W = L + n;                                     // [n] the log weights
  const LooCell c = loo_cell<COLS>(a);
  double* o = a.out + (long)c.cell * kLooFields;
  // ---- the ratios, the tail and the log weight of every draw
  CellRatios cr;
  if (loo_cell_verdict<COLS, true>(a, c, m, L, sh, &cr) == CELL_NAN) {
    if (tid == 0) o[0] = o[1] = o[2] = o[3] = NAN;
    return;
  }
  const double khat = loo_cell_weights<false>(a, c, m, cr, W, sh);
  // ---- logsumexp(lw + ll) - logsumexp(lw) over the draws that take part; lpd = logsumexp(ll) - log N
  auto part = [&](long i) { return V[i] != -INFINITY; };
  const double ma = draws_max(n, sh.red, [&](long i) { return part(i) ? W[i] + L[i] : -INFINITY; });
  const double mb = draws_max(n, sh.red, [&](long i) { return part(i) ? W[i] : -INFINITY; });
  const double sa = draws_sum(n, sh.red, [&](long i) { return part(i) ? exp(W[i] + L[i] - ma) : 0.0; });
  const double sb = draws_sum(n, sh.red, [&](long i) { return part(i) ? exp(W[i] - mb) : 0.0; });
  const double elpd = loo_ap_lse(ma, sa) - loo_ap_lse(mb, sb);
  double p_loo = 0.0;
  if (!c.excluded) {
    const double sl = draws_sum(n, sh.red, [&](long i) { return part(i) ? exp(L[i] - cr.lmax) : 0.0; });
    p_loo = loo_ap_lse(cr.lmax, sl) - log((double)cr.N) - elpd;
  }
  if (tid == 0) { o[0] = elpd; o[1] = p_loo; o[2] = -2.0 * elpd; o[3] = khat; }
}

// ---- launch helpers (host)
int loo_sel_pad(long n, double r_eff_min) { return pow2_at_least((long)psis_tail_len(n, r_eff_min) + 1); }
hipError_t launch_loo_table_kernel(const double* draws, long n_draws, const Dims& d, const int* genes, int n_genes, double* T,
                                   hipStream_t st) {
  dim3 grid((unsigned)((n_draws + 31) / 32), (unsigned)((n_genes + 31) / 32));
  hipLaunchKernelGGL(ppcx_loo_table_kernel, grid, dim3(256), 0, st, draws, n_draws, d, genes, n_genes, T);
  return hipGetLastError();
}
hipError_t launch_loo_ll_kernel(const LooArgs& a, long j0, long n_rows, double* out, hipStream_t st) {
  const long total = n_rows * (long)a.n_cells;
  hipLaunchKernelGGL(ppcx_loo_ll_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, j0, n_rows, out);
  return hipGetLastError();
}
PPCX_KERNEL_OF(ppcx_loo_kernel);
PPCX_KERNEL_OF(ppcx_loo_ap_kernel);
// doubles per cell of the kernel that launch_loo_kernel picks
static long loo_slice(const LooArgs& a) { return a.lr ? loo_ap_slice(a.n) : a.n; }
// fields: kLooFields, or kLooMcseFields (a.out then holds six per cell); with a.lr the approximate-posterior kernel (kLooFields)
hipError_t launch_loo_kernel(const LooArgs& a, int fields, int n_blocks, hipStream_t st) {
  const CellLaunch c = cell_launch(a, n_blocks);
  if (a.lr && fields != kLooFields) return hipErrorInvalidValue;
  void (*const kernel)(LooArgs) = a.lr ? pick_kernel<ppcx_loo_ap_kernel_of>(c.lds, c.cols)
                                       : pick_kernel<ppcx_loo_kernel_of>(c.lds, c.cols, fields == kLooMcseFields);
  return launch_cell_kernel(kernel, a, c, a.sel_pad, loo_slice(a), st);
}

// Cells of a launch in batches: all at once where the ratios live in LDS, else as many as the scratch bound holds.
static hipError_t loo_cells(const LooArgs& args, int fields, int n_cells, size_t scratch_bytes, DeviceBuffer<double>& scratch, hipStream_t st) {
  return cells_in_batches(args, loo_slice(args), n_cells, scratch_bytes, scratch, [&](const LooArgs& a, const CellLaunch& c) {
    return launch_loo_kernel(a, fields, c.n_blocks, st);
  });
}

// what both walks run per batch: the LOO kernel over the batch's cells
static auto loo_body(int fields, size_t scratch_bytes, hipStream_t st) {
  return [=](const LooArgs& a, const int*, int n_cells, DeviceBuffer<double>& scratch) {
    return loo_cells(a, fields, n_cells, scratch_bytes, scratch, st);
  };
}
hipError_t loo_fit_cells(const FitCells& fc, int fields, double* out, size_t scratch_bytes, hipStream_t st) {
  return for_gene_batches(fc, fields, out, scratch_bytes, st, loo_body(fields, scratch_bytes, st));
}
hipError_t loo_columns(const GivenCells& gc, int fields, double* out, size_t scratch_bytes, hipStream_t st) {
  return for_given_columns(gc, fields, out, st, loo_body(fields, scratch_bytes, st));
}

hipError_t loo_fit_log_lik(const FitCells& fc, double* out, size_t scratch_bytes, hipStream_t st) {
  const size_t ncells = (size_t)fc.n_genes * fc.d.S;
  const long n = fc.n;
  // the whole table of the requested genes, then the matrix in row blocks of at most scratch_bytes
  long rows = (long)std::max<size_t>(1, scratch_bytes / (sizeof(double) * ncells));
  if (rows > n) rows = n;
  FitCellsDev dev; DeviceBuffer<double> d_T, d_buf;
  hipError_t e = dev.upload(fc, st);
  if (e == hipSuccess) e = d_T.alloc((size_t)(fc.d.C + 1) * (size_t)n * fc.n_genes);
  if (e == hipSuccess) e = d_buf.alloc(ncells * (size_t)rows);
  if (e == hipSuccess) e = launch_loo_table_kernel(fc.draws, n, fc.d, dev.genes.p, fc.n_genes, d_T.p, st);
  const LooArgs a = dev.args(fc, d_T.p, 0, fc.n_genes);
  for (long j0 = 0; e == hipSuccess && j0 < n; j0 += rows) {
    const long nr = n - j0 < rows ? n - j0 : rows;
    e = launch_loo_ll_kernel(a, j0, nr, d_buf.p, st);
    if (e == hipSuccess) e = d_buf.download(out + (size_t)j0 * ncells, ncells * (size_t)nr, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // d_buf is rewritten by the next block
  }
  return finish(e, st);
}

}  // namespace ppcx
