// ppcx_loo_mm_split.hip -- gfx950 kernel of the split transformation of gene-local moment matching (ppcx_fit_loo_moment_match_split,
// ppcx_fit_loo_predict_exact_moment_match_split, include/ppcx.h; the statistic: ppcx_loo_mm_split.h). The walk over the cells is
// ppcx_loo_dev.h's (for_gene_batches, cells_in_batches); the driver is ppcx_loo_mm_dev.h's (loo_mm_then_fit_cells): per batch of
// cells ppcx_loo_kernel and ppcx_loo_mm_kernel as ppcx_fit_loo_moment_match launches them, into a device record that never
// leaves the device, then the kernel below.
//
//   ppcx_loo_mm_split_kernel  one workgroup of kBlockThreads per cell; PRED: the predictive form. It reads the cell's iterations,
//                             scale and shift from the matching's record and copies the record (PRED: its tail behind the ten
//                             fields). The branch on iterations is on a word every thread reads from the same address: the
//                             control flow is uniform per workgroup.
//                             iterations == 0: the elpd form leaves before a ratio is formed; the predictive form calls
//                             loo_exact_cell (ppcx_loo_dev.h), the function that ppcx_loo_exact_kernel is, as
//                             ppcx_loo_mm_exact_kernel's unmatched path does: the ten fields are its bits by construction.
//                             iterations > 0: the states (A, B), the identity and (Ainv, Binv) in LDS, written by tid < nc before
//                             a barrier. Per draw the lane selects two state pointers -- ((A, B), identity) below h = n / 2,
//                             (identity, (Ainv, Binv)) from h on -- and loo_mm_split_ratio calls loo_mm_density at its two fixed
//                             sites: h falls inside a wavefront for most n, and a branch per half would inline the density at
//                             four; the selection stands inside the one sweep of loo_mm_count_ratios. The tail and the weights
//                             by loo_cell_tail and loo_cell_lw, the matching's own calls. The elpd form keeps ll_x and ends in
//                             loo_mm_weighted_elpd, ppcx_loo_mm_kernel's step 4; lpd of the original draws is formed first by
//                             that kernel's loo_cell_ratios and loo_mm_lpd (into the ratios' place). The predictive form puts
//                             (eta, ln phi) at the proposal points in the ratios' place (loo_fill_eta_lnphi) and ends in
//                             ppc_exact_sweeps over ExactBlockSums.
//                             Three arrays of n doubles -- ratio (then eta), log weight (then weight), ll_x or ln phi -- in LDS
//                             up to kPsisLdsDraws draws beside the two selection arrays (96 KB + 4 KB at 4 096 draws: one
//                             workgroup per CU; 1 000 draws take 24 KB + 2 KB), in the workgroup's slice of the bounded scratch
//                             beyond. Timed at the entry only (profiles/README.md, cell_entries_ab.json).
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_split.h"

namespace ppcx {

struct LooMmSplitShared { double A[kMaxC + 1], B[kMaxC + 1], Ainv[kMaxC + 1], Binv[kMaxC + 1], one[kMaxC + 1], zero[kMaxC + 1]; };

template <bool LDS, bool PRED>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_split_kernel(LooMmThenArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmSplitShared ms;
  const LooArgs& a = p.m.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_slice3(n));
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
    // ---- the predictive form of a cell that was not matched: ppcx_loo_exact_kernel's cell
    if constexpr (PRED) loo_exact_cell<false, false>(a, c, m, nullptr, nullptr, p.log_tc, p.p_lo, p.p_hi, o, sh);
    return;
  }
  // ---- the elpd form: lpd of the original draws, as ppcx_loo_mm_kernel forms it
  double lpd = NAN;
  if constexpr (!PRED) {
    CellRatios cr;
    if (loo_cell_ratios<false, false>(a, c, false, m.V, nullptr, sh, &cr)) { all_nan(); return; }
    const double l = loo_mm_lpd(m.V, n, cr, sh);
    lpd = cr.N > 0 ? l : NAN;
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
  const CountedRatios cr = loo_mm_count_ratios(n, m.V, sh, [&](long i) {
    const bool first = i < h;
    const double* Ax = first ? ms.A : ms.one;
    const double* Bx = first ? ms.B : ms.zero;
    const double* Ai = first ? ms.one : ms.Ainv;
    const double* Bi = first ? ms.zero : ms.Binv;
    double lx;
    const double r = loo_mm_split_ratio(g, i, Ax, Bx, Ai, Bi, logJ, s, &lx);
    if constexpr (!PRED) LP[i] = lx;
    return r;
  });
  if (cr.N == 0) { all_nan(); return; }
  // ---- step 6
  const int M = psis_tail_len(cr.N, a.r_eff ? a.r_eff[cell] : 1.0);
  const LooTail lt = loo_cell_tail(m.V, n, cr.N, M, m.K, m.X, a.sel_pad, sh);
  if constexpr (!PRED) {
    // ---- step 7, ppcx_loo_mm_kernel's step 4 with ll_x as kept (a thread reads the log weights and ll_x it wrote itself)
    loo_cell_lw<false>(m.V, W, n, cr.rmax, lt, M, m.K, sh);
    const double elpd = loo_mm_weighted_elpd(W, n, sh, [&](long i) { return LP[i]; });
    if (tid == 0) loo_mm_split_store(o, C, elpd, lpd, lt.khat);
  } else {
    // ---- step 8: the normalised weights; (eta, ln phi) at the proposal points, eta into the ratios' place
    loo_cell_lw<true>(m.V, W, n, cr.rmax, lt, M, m.K, sh);
    __syncthreads();                                     // no thread reads a ratio any more: V becomes E
    const bool inval = loo_fill_eta_lnphi(n, p.log_tc, E, LP, [&](long i, double* sg) {
      const bool first = i < h;
      return loo_mm_exact_eta(g, s, i, first ? ms.A : ms.one, first ? ms.B : ms.zero, sg);
    });
    if (inval) { all_nan(); return; }
    const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, y, excluded, 1, p.p_lo, p.p_hi, tid == 0, o);
    if (tid == 0) { o[kPpcExactFields] = ok ? rec[3] : NAN; *ks = ok ? lt.khat : NAN; }
  }
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_split_kernel);

// the elpd form takes tc = 1 and leaves the probabilities unread
hipError_t loo_mm_split_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool predictive, double tc, double p_lo,
                                  double p_hi, double* out, size_t scratch_bytes, hipStream_t st) {
  const int fields = predictive ? loo_mm_exact_split_fields(fc.d.C) : loo_mm_split_fields(fc.d.C);
  return loo_mm_then_fit_cells(fc, LooMmDiagMatching{}, k_threshold, max_iters, predictive ? tc : 1.0, p_lo, p_hi, fields, out, scratch_bytes,
                               st, [=](bool lds) { return pick_kernel<ppcx_loo_mm_split_kernel_of>(lds, predictive); });
}

}  // namespace ppcx
