// ppcx_loo_mm_split.hip -- gfx950 kernel of the split transformation of gene-local moment matching (ppcx_fit_loo_moment_match_split,
// ppcx_fit_loo_predict_exact_moment_match_split, include/ppcx.h; the statistic: ppcx_loo_mm_split.h). The walk over the cells is
// ppcx_loo_dev.h's (for_gene_batches, cells_in_batches); the driver at the end of this file launches, per batch of cells,
// ppcx_loo_kernel and ppcx_loo_mm_kernel as ppcx_fit_loo_moment_match does (launch_loo_mm_kernels, ppcx_loo_mm_dev.h) into a device
// record that never leaves the device, then the kernel below.
//
//   ppcx_loo_mm_split_kernel  one workgroup of kBlockThreads per cell; PRED: the predictive form. It reads the cell's iterations,
//                             scale and shift from the matching's record and copies the record (PRED: its tail behind the ten
//                             fields). The branch on iterations is on a word every thread reads from the same address: the
//                             control flow is uniform per workgroup.
//                             iterations == 0: the elpd form leaves before a ratio is formed; the predictive form runs
//                             ppcx_loo_exact_kernel's own stages as ppcx_loo_mm_exact_kernel's unmatched path does, so the ten
//                             fields are its bits.
//                             iterations > 0: the states (A, B), the identity and (Ainv, Binv) in LDS, written by tid < nc before
//                             a barrier. Per draw the lane selects two state pointers -- ((A, B), identity) below h = n / 2,
//                             (identity, (Ainv, Binv)) from h on -- and loo_mm_split_ratio calls loo_mm_density at its two fixed
//                             sites: h falls inside a wavefront for most n, and a branch per half would inline the density at
//                             four. The tail and the weights by loo_cell_tail and loo_cell_lw, the matching's own calls.
//                             The elpd form keeps ll_x and ends as ppcx_loo_mm_kernel's step 4; lpd of the original draws is
//                             formed first as that kernel forms it (loo_cell_ratios into the ratios' place). The predictive
//                             form puts (eta, ln phi) at the proposal points in the ratios' place and ends in ppc_exact_sweeps
//                             over ExactBlockSums.
//                             Three arrays of n doubles -- ratio (then eta), log weight (then weight), ll_x or ln phi -- in LDS
//                             up to kPsisLdsDraws draws beside the two selection arrays (96 KB + 4 KB at 4 096 draws: one
//                             workgroup per CU; 1 000 draws take 24 KB + 2 KB), in the workgroup's slice of the bounded scratch
//                             beyond. Not timed.
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_split.h"

namespace ppcx {

struct LooMmSplitArgs {
  LooMmArgs m;                     // the matching's block: m.l the table and the cells, m.out its record [cells][loo_mm_fields(C)] (device)
  double log_tc = 0.0, p_lo = 0.025, p_hi = 0.975;   // the predictive form's
  double* out = nullptr;           // [cells][loo_mm_split_fields(C)], the predictive form [cells][loo_mm_exact_split_fields(C)]
};
inline LooArgs& cell_args(LooMmSplitArgs& p) { return p.m.l; }

// doubles per cell, in LDS or in the scratch: ratio / eta [n], log weight / weight [n], ll_x or ln phi [n]. The matching's
// kernels run before it in slices of their own size from the same scratch, so a batch is sized by the larger of the two.
__host__ __device__ inline long loo_mm_split_slice(long n) { return 3 * n; }

struct LooMmSplitShared { double A[kMaxC + 1], B[kMaxC + 1], Ainv[kMaxC + 1], Binv[kMaxC + 1], one[kMaxC + 1], zero[kMaxC + 1]; };

template <bool LDS, bool PRED>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_split_kernel(LooMmSplitArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmSplitShared ms;
  const LooArgs& a = p.m.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_mm_split_slice(n));
  double* W = m.V + n;                                   // [n] log weights, then weights (m.V: [n] the ratios)
  double* LP = W + n;                                    // [n] ll_x; the predictive form: ln phi
  double* E = m.V;                                       // [n] eta, once the ratios are dead
  const LooCell c = loo_cell<false>(a);
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  const bool excluded = c.excluded;
  double* o = p.out + (long)cell * (PRED ? loo_mm_exact_split_fields(C) : loo_mm_split_fields(C));
  const double* rec = p.m.out + (long)cell * loo_mm_fields(C);
  const bool matched = rec[5] > 0.0;                     // uniform: every thread reads the same word
  double* ks = PRED ? o + loo_mm_exact_fields(C) : nullptr;   // the predictive form's khat_split
  if (tid == 0) {
    if constexpr (PRED) { loo_mm_exact_store_state(o, C, rec); *ks = NAN; }
    else loo_mm_split_store_record(o, C, rec);
  }
  auto all_nan = [&]() {
    if (tid != 0) return;
    if constexpr (PRED) loo_exact_store_nan(o, y, excluded);
    else loo_mm_split_store_nan(o, C);
  };
  if (!matched) {
    if constexpr (PRED) {
      // ---- ppcx_loo_exact_kernel's stages, as ppcx_loo_mm_exact_kernel's unmatched path runs them
      double khat = NAN;
      bool inval = false;
      CellRatios cr;
      const CellVerdict verdict = loo_cell_verdict<false, false>(a, c, m, nullptr, sh, &cr);
      if (verdict == CELL_NAN) { all_nan(); return; }
      const bool uniform = verdict == CELL_UNIFORM;      // already held out: w_i = 1, every sum over n
      if (uniform) for (long i = tid; i < n; i += kBlockThreads) W[i] = 1.0;
      else khat = loo_cell_weights<true>(a, c, m, cr, W, sh);
      __syncthreads();                                   // no thread reads a ratio any more: V becomes E
      const double* Tg = a.T + (long)gi * nc * n;
      for (long i = tid; i < n; i += kBlockThreads) {
        double sg = 0.0;
        const double eta = loo_cell_eta(a, Tg, s, i, &sg);
        const double lp = ppc_exact_lnphi(sg, p.log_tc);
        E[i] = eta; LP[i] = lp;
        inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
      }
      if (block_any(inval)) { all_nan(); return; }
      const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, y, excluded, uniform ? n : 1, p.p_lo, p.p_hi, tid == 0, o);
      if (tid == 0) o[kPpcExactFields] = ok ? khat : NAN;
    }
    return;
  }
  // ---- the elpd form: lpd of the original draws, as ppcx_loo_mm_kernel forms it
  double lpd = NAN;
  if constexpr (!PRED) {
    CellRatios cr;
    if (loo_cell_ratios<false, false>(a, c, false, m.V, nullptr, sh, &cr)) { all_nan(); return; }
    const double lmax = cr.lmax;
    const double sl = draws_sum(n, sh.red, [&](long i) { const double r = m.V[i]; return r != -INFINITY ? exp(-r - lmax) : 0.0; });
    lpd = cr.N > 0 ? (lmax == -INFINITY ? -INFINITY : lmax + log(sl)) - log((double)cr.N) : NAN;
  }
  // ---- step 2: the three states
  const LooMmGene g = loo_mm_gene(p.m, gi);
  if (tid < nc) {
    const double* A = rec + kLooMmHead;
    const double* B = A + nc;
    ms.A[tid] = A[tid]; ms.B[tid] = B[tid]; ms.one[tid] = 1.0; ms.zero[tid] = 0.0;
    ms.Ainv[tid] = loo_mm_split_Ainv(g, tid, A); ms.Binv[tid] = loo_mm_split_Binv(g, tid, A, B);
  }
  __syncthreads();
  const double logJ = loo_mm_split_logJ(g, ms.A);        // every thread the same sum
  const long h = loo_mm_split_half(n);
  // ---- steps 3 - 5: the ratios, two state pointers per lane and two fixed sites of the density
  double cnt = 0.0, rmx = -INFINITY;
  for (long i = tid; i < n; i += kBlockThreads) {
    const bool first = i < h;
    const double* Ax = first ? ms.A : ms.one;
    const double* Bx = first ? ms.B : ms.zero;
    const double* Ai = first ? ms.one : ms.Ainv;
    const double* Bi = first ? ms.zero : ms.Binv;
    double lx;
    const double r = loo_mm_split_ratio(g, i, Ax, Bx, Ai, Bi, logJ, s, &lx);
    if (r != -INFINITY) { cnt += 1.0; rmx = fmax(rmx, r); }
    m.V[i] = r;
    if constexpr (!PRED) LP[i] = lx;
  }
  const long N = (long)block_sum(cnt, sh.red);
  rmx = block_max(rmx, sh.red);
  if (N == 0) { all_nan(); return; }
  // ---- step 6
  const int M = psis_tail_len(N, a.r_eff ? a.r_eff[cell] : 1.0);
  const LooTail lt = loo_cell_tail(m.V, n, N, M, m.K, m.X, a.sel_pad, sh);
  if constexpr (!PRED) {
    // ---- step 7, as ppcx_loo_mm_kernel's step 4 (a thread reads the log weights and ll_x it wrote itself)
    loo_cell_lw<false>(m.V, W, n, rmx, lt, M, m.K, sh);
    double ma = -INFINITY, mb = -INFINITY;
    for (long i = tid; i < n; i += kBlockThreads) {
      const double lw = W[i];
      if (lw == -INFINITY) continue;
      ma = fmax(ma, lw + LP[i]); mb = fmax(mb, lw);
    }
    ma = block_max(ma, sh.red);
    mb = block_max(mb, sh.red);
    double sa = 0.0, sb = 0.0;
    for (long i = tid; i < n; i += kBlockThreads) {
      const double lw = W[i];
      if (lw == -INFINITY) continue;
      sa += exp(lw + LP[i] - ma); sb += exp(lw - mb);
    }
    sa = block_sum(sa, sh.red);
    sb = block_sum(sb, sh.red);
    const double elpd = loo_ap_lse(ma, sa) - loo_ap_lse(mb, sb);
    if (tid == 0) loo_mm_split_store(o, C, elpd, lpd, lt.khat);
  } else {
    // ---- step 8: the normalised weights; (eta, ln phi) at the proposal points, eta into the ratios' place
    loo_cell_lw<true>(m.V, W, n, rmx, lt, M, m.K, sh);
    __syncthreads();                                     // no thread reads a ratio any more: V becomes E
    bool inval = false;
    for (long i = tid; i < n; i += kBlockThreads) {
      const bool first = i < h;
      double sg;
      const double eta = loo_mm_exact_eta(g, s, i, first ? ms.A : ms.one, first ? ms.B : ms.zero, &sg);
      const double lp = ppc_exact_lnphi(sg, p.log_tc);
      E[i] = eta; LP[i] = lp;
      inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
    }
    if (block_any(inval)) { all_nan(); return; }
    const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, y, excluded, 1, p.p_lo, p.p_hi, tid == 0, o);
    if (tid == 0) { o[kPpcExactFields] = ok ? rec[3] : NAN; *ks = ok ? lt.khat : NAN; }
  }
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_split_kernel);

hipError_t loo_mm_split_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool predictive, double tc, double p_lo,
                                  double p_hi, double* out, size_t scratch_bytes, hipStream_t st) {
  const long n = fc.n;
  const int mm_fields = loo_mm_fields(fc.d.C);
  LooMmWalk walk; DeviceBuffer<double> d_rec;            // outlive the walk, which drains the stream before it returns
  hipError_t e = walk.prepare(fc, st);
  if (e == hipSuccess) e = d_rec.alloc((size_t)fc.n_genes * fc.d.S * mm_fields);
  if (e != hipSuccess) return finish(e, st);
  const double log_tc = predictive ? log(tc) : 0.0;
  return for_gene_batches(fc, predictive ? loo_mm_exact_split_fields(fc.d.C) : loo_mm_split_fields(fc.d.C), out, scratch_bytes, st,
                          [&](const LooArgs& a, const int* genes, int n_cells, DeviceBuffer<double>& scratch) {
    LooMmSplitArgs p;
    const size_t done = walk.done;
    p.m = walk.args(fc, a, genes, n_cells, k_threshold, max_iters, d_rec.p + done * mm_fields);
    p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi; p.out = a.out;
    // per batch of cells: plain PSIS-LOO and the matching into the device record, then the split under its state
    const long slice = loo_mm_split_slice(n) > loo_mm_slice(n) ? loo_mm_split_slice(n) : loo_mm_slice(n);
    return cells_in_batches(p, slice, n_cells, scratch_bytes, scratch, [&](const LooMmSplitArgs& q, const CellLaunch& c) {
      const hipError_t e1 = launch_loo_mm_kernels(q.m, c, st);
      return e1 == hipSuccess ? launch_cell_kernel(pick_kernel<ppcx_loo_mm_split_kernel_of>(c.lds, predictive), q, c, q.m.l.sel_pad, slice, st)
                              : e1;
    });
  });
}

}  // namespace ppcx
