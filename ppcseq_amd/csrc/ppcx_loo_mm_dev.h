// ppcx_loo_mm_dev.h -- what the kernels over moment-matched cells share (ppcx_loo_mm.hip: the matching itself;
// ppcx_loo_mm_exact.hip: the exact predictive under the matched weights; ppcx_loo_mm_split.hip: the split transformation, both
// forms). On the device: the argument block of the matching and the one of a kernel that runs after it (LooMmThenArgs), the gene
// a workgroup reads, and the stages that more than one of the kernels runs -- the counted sweep of a state's ratios
// (loo_mm_count_ratios), lpd of the original draws (loo_mm_lpd), the weighted elpd (loo_mm_weighted_elpd) and the normaliser of
// the current weights (loo_mm_lse). The unmatched
// predictive cell and the fill of (eta, ln phi) are ppcx_loo_dev.h's (loo_exact_cell, loo_fill_eta_lnphi), shared with
// ppcx_loo_exact_kernel. On the host: what a walk of the matching keeps on the device beside for_gene_batches' own buffers, the
// launch of plain PSIS-LOO and the matching over a batch of cells, and the one driver of the entries that launch a kernel
// after them (loo_mm_then_fit_cells). Every kernel of the family keeps three arrays of n doubles per cell: loo_slice3.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_loo_dev.h"
#include "ppcx_loo_mm.h"

namespace ppcx {

struct LooMmArgs {
  LooArgs l;                       // the table, y, r_eff, n, the cells, sel_pad, the scratch of both kernels (l.out: ppcx_loo_kernel's)
  const int* genes = nullptr;      // [table's genes] their ids in the model (device)
  const double* U = nullptr;       // [6][n] ppcx_loo_mm_hyper_kernel
  const double* loo = nullptr;     // [cells][kLooFields] ppcx_loo_kernel's fields of the table's cells
  int K = 0;                       // checked genes of the model
  double lambda_mu_mu = 0.0, k_threshold = 0.7;
  int max_iters = 0;
  double* out = nullptr;           // [cells][loo_mm_fields(C)]; ppcx_loo_mm_cov_kernel: [cells][loo_mm_cov_fields(C)]
  double* inv = nullptr;           // ppcx_loo_mm_cov_kernel<.., INV>, optional: [cells][(C + 1)^2 + (C + 1) + 1] Minv, binv, logJ of a matched cell
};

// The argument block of a kernel that runs after the matching over the same cells (ppcx_loo_mm_exact_kernel,
// ppcx_loo_mm_split_kernel, ppcx_loo_mm_cov_exact_kernel)
struct LooMmThenArgs {
  LooMmArgs m;                     // the matching's block: m.l the table and the cells, m.out its record (device), m.inv its second one
  double log_tc = 0.0, p_lo = 0.025, p_hi = 0.975;   // the predictive forms'
  double* out = nullptr;           // [cells][the entry's fields]
};
inline LooArgs& cell_args(LooMmThenArgs& p) { return p.m.l; }

// gene gi of the table as the local density reads it
__device__ __forceinline__ LooMmGene loo_mm_gene(const LooMmArgs& p, int gi) {
  const LooArgs& a = p.l;
  LooMmGene g;
  g.Tg = a.T + (long)gi * (a.C + 1) * a.n; g.U = p.U; g.n = a.n; g.C = a.C; g.S = a.S;
  g.checked = a.C >= 2 && p.genes[gi] < p.K;
  g.yrow = a.y + (long)gi * a.S; g.expo = a.expo; g.X = a.X; g.lambda_mu_mu = p.lambda_mu_mu;
  return g;
}

// The ratio of every draw under a state into V[0 .. n), r_i = ratio(i), counted: N the draws that are not -Inf and the largest
// ratio. Every thread gets the same. The density's call sites are the caller's, inside `ratio`.
struct CountedRatios { long N; double rmax; };
template <class F>
__device__ __forceinline__ CountedRatios loo_mm_count_ratios(long n, double* V, PsisShared& sh, F ratio) {
  PPCX_NO_CONTRACT
  double cnt = 0.0, rmx = -INFINITY;
  for (long i = threadIdx.x; i < n; i += kBlockThreads) {
    const double r = ratio(i);
    if (r != -INFINITY) { cnt += 1.0; rmx = fmax(rmx, r); }
    V[i] = r;
  }
  const long N = (long)block_sum(cnt, sh.red);
  rmx = block_max(rmx, sh.red);
  return CountedRatios{N, rmx};
}

// lpd of the original draws from their ratios V = -ll and loo_cell_ratios' CellRatios: log mean exp ll over the cr.N draws
// that take part. What becomes of a cell with cr.N == 0 is the caller's.
__device__ __forceinline__ double loo_mm_lpd(const double* V, long n, const CellRatios& cr, PsisShared& sh) {
  PPCX_NO_CONTRACT
  const double lmax = cr.lmax;
  const double sl = draws_sum(n, sh.red, [&](long i) { const double r = V[i]; return r != -INFINITY ? exp(-r - lmax) : 0.0; });
  return (lmax == -INFINITY ? -INFINITY : lmax + log(sl)) - log((double)cr.N);
}

// elpd_loo = logsumexp(lw + ll) - logsumexp(lw) over the draws with a log weight W[i] above -Inf, ll(i) the cell's
// log-likelihood at draw i (ppcx_loo_mm.h step 4, ppcx_loo_mm_split.h step 7): the two maxima, then the two sums. A thread
// reads the log weights it wrote itself.
template <class F>
__device__ __forceinline__ double loo_mm_weighted_elpd(const double* W, long n, PsisShared& sh, F ll) {
  PPCX_NO_CONTRACT
  const int tid = threadIdx.x;
  double ma = -INFINITY, mb = -INFINITY;
  for (long i = tid; i < n; i += kBlockThreads) {
    const double lw = W[i];
    if (lw == -INFINITY) continue;
    ma = fmax(ma, lw + ll(i)); mb = fmax(mb, lw);
  }
  ma = block_max(ma, sh.red);
  mb = block_max(mb, sh.red);
  double sa = 0.0, sb = 0.0;
  for (long i = tid; i < n; i += kBlockThreads) {
    const double lw = W[i];
    if (lw == -INFINITY) continue;
    sa += exp(lw + ll(i) - ma); sb += exp(lw - mb);
  }
  sa = block_sum(sa, sh.red);
  sb = block_sum(sb, sh.red);
  return loo_ap_lse(ma, sa) - loo_ap_lse(mb, sb);
}

// The normaliser of the current weights: logsumexp of the log weights W[0 .. n). Every thread gets the same.
__device__ __forceinline__ double loo_mm_lse(const double* W, long n, PsisShared& sh) {
  const double mb = draws_max(n, sh.red, [&](long i) { return W[i]; });
  const double sb = draws_sum(n, sh.red, [&](long i) { return exp(W[i] - mb); });
  return mb + log(sb);
}

// ---- host (ppcx_loo_mm.hip)
// What a walk of the matching keeps for all of its gene batches: the draws' transposed hyper-parameters and ppcx_loo_kernel's
// fields of every cell. prepare() before for_gene_batches; args() once per gene batch, in the walk's order (it counts the cells
// of the earlier batches): the batch's LooMmArgs with the matching's record [cells][loo_mm_fields(C)] at `out` (device).
struct LooMmWalk {
  DeviceBuffer<double> U, loo;
  size_t done = 0;
  hipError_t prepare(const FitCells& fc, hipStream_t st);
  LooMmArgs args(const FitCells& fc, const LooArgs& a, const int* genes, int n_cells, double k_threshold, int max_iters, double* out);
};
// plain PSIS-LOO by its own kernel (its slices of the scratch lie within the matching's), then the matching, over the launch c
hipError_t launch_loo_mm_kernels(const LooMmArgs& q, const CellLaunch& c, hipStream_t st);
// the same with the matching of ppcx_loo_mm_cov.hip (split: its split instantiation)
hipError_t launch_loo_mm_cov_kernels(const LooMmArgs& q, const CellLaunch& c, bool split, hipStream_t st);

// The matching that runs ahead of a kernel, as loo_mm_then_fit_cells takes it: its launch over a batch of cells, the width of
// its record and of an optional second device record per cell (0: none; LooMmArgs::inv). The per-coordinate matching:
struct LooMmDiagMatching {
  int fields(int C) const { return loo_mm_fields(C); }
  int second(int) const { return 0; }
  hipError_t launch(const LooMmArgs& q, const CellLaunch& c, hipStream_t st) const { return launch_loo_mm_kernels(q, c, st); }
};

// The driver of an entry that is the matching itself, with either state: per batch of cells launch(q, c) -- plain PSIS-LOO, then
// the matching's kernel -- with `fields` doubles per cell into out (host)
template <class Launch>
hipError_t loo_mm_match_cells(const FitCells& fc, double k_threshold, int max_iters, int fields, double* out, size_t scratch_bytes,
                              hipStream_t st, Launch launch) {
  LooMmWalk walk;                                        // outlives the walk, which drains the stream before it returns
  const hipError_t e = walk.prepare(fc, st);
  if (e != hipSuccess) return finish(e, st);
  return for_gene_batches(fc, fields, out, scratch_bytes, st,
                          [&](const LooArgs& a, const int* genes, int n_cells, DeviceBuffer<double>& scratch) {
    const LooMmArgs p = walk.args(fc, a, genes, n_cells, k_threshold, max_iters, a.out);
    return cells_in_batches(p, loo_slice3(fc.n), n_cells, scratch_bytes, scratch, launch);
  });
}

// The driver of an entry that runs a kernel after a matching `mt` (LooMmDiagMatching, ppcx_loo_mm_cov_exact.hip's): per batch of
// cells plain PSIS-LOO and the matching into a device record (and its optional second one) that never leaves the device, then
// then(c.lds) -- the kernel's instantiation for cells in LDS or in the scratch -- with `fields` doubles per cell into out (host).
// Every kernel takes its slice of loo_slice3 doubles from the same scratch.
template <class Matching, class Then>
hipError_t loo_mm_then_fit_cells(const FitCells& fc, const Matching& mt, double k_threshold, int max_iters, double tc, double p_lo,
                                 double p_hi, int fields, double* out, size_t scratch_bytes, hipStream_t st, Then then) {
  const int mm_fields = mt.fields(fc.d.C), inv_fields = mt.second(fc.d.C);
  LooMmWalk walk; DeviceBuffer<double> d_rec, d_inv;     // outlive the walk, which drains the stream before it returns
  hipError_t e = walk.prepare(fc, st);
  if (e == hipSuccess) e = d_rec.alloc((size_t)fc.n_genes * fc.d.S * mm_fields);
  if (e == hipSuccess && inv_fields > 0) e = d_inv.alloc((size_t)fc.n_genes * fc.d.S * inv_fields);
  if (e != hipSuccess) return finish(e, st);
  const double log_tc = log(tc);
  const long slice = loo_slice3(fc.n);
  return for_gene_batches(fc, fields, out, scratch_bytes, st,
                          [&](const LooArgs& a, const int* genes, int n_cells, DeviceBuffer<double>& scratch) {
    LooMmThenArgs p;
    const size_t done = walk.done;
    p.m = walk.args(fc, a, genes, n_cells, k_threshold, max_iters, d_rec.p + done * mm_fields);
    if (inv_fields > 0) p.m.inv = d_inv.p + done * inv_fields;
    p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi; p.out = a.out;
    return cells_in_batches(p, slice, n_cells, scratch_bytes, scratch, [&](const LooMmThenArgs& q, const CellLaunch& c) {
      const hipError_t e1 = mt.launch(q.m, c, st);
      return e1 == hipSuccess ? launch_cell_kernel(then(c.lds), q, c, q.m.l.sel_pad, slice, st) : e1;
    });
  });
}

}  // namespace ppcx
