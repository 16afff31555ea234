// ppcx_loo_mm_cov_exact.hip -- gfx950 kernel of the exact leave-one-out predictive tails and interval per cell under the weights of
// the matching with the covariance step (ppcx_fit_loo_predict_exact_moment_match_cov, include/ppcx.h; the statistic:
// ppcx_loo_mm_cov_exact.h). The walk over the cells is ppcx_loo_dev.h's (for_gene_batches, cells_in_batches); the driver is
// ppcx_loo_mm_dev.h's (loo_mm_then_fit_cells) under the matching below: per batch of cells ppcx_loo_kernel and the non-split
// ppcx_loo_mm_cov_kernel as ppcx_fit_loo_moment_match_cov launches them, into a device record and, beside it, the accumulated
// inverse (LooMmArgs::inv) -- neither leaves the device -- then the kernel below.
//
//   ppcx_loo_mm_cov_exact_kernel  one workgroup of kBlockThreads per cell; SPLIT: under the split transformation. It mirrors
//                                 ppcx_loo_mm_exact_kernel and the PRED branch of ppcx_loo_mm_split_kernel step for step, under the
//                                 affine state. It reads the cell's iterations from the matching's record and copies the record's
//                                 tail behind its ten fields. The branch on iterations is on a word every thread reads from the
//                                 same address: the control flow is uniform per workgroup.
//                                 iterations == 0: loo_exact_cell (ppcx_loo_dev.h), the function that ppcx_loo_exact_kernel is.
//                                 iterations > 0: (M, b), the identity state and, SPLIT, (Minv, binv) and logJ in static LDS
//                                 (LooMmCovExactShared: three (C + 1)^2 matrices at kMaxC), written before a barrier. Unsplit: per
//                                 draw q(t; h) and Q0 by loo_mm_density under LooMmAffine in one visit. SPLIT: per draw the lane
//                                 selects two state pointers -- ((M, b), identity) below h = n / 2, (identity, (Minv, binv)) from h
//                                 on -- and loo_mm_split_ratio calls the density at its two fixed sites, as ppcx_loo_mm_cov_kernel's
//                                 step 7 does. The ratios go through loo_mm_count_ratios, the tail and the normalised weights
//                                 through loo_cell_tail and loo_cell_lw, the matching's own calls; then (eta, ln phi) at the
//                                 proposal points, eta into the ratios' place (loo_fill_eta_lnphi), and ppc_exact_sweeps over
//                                 ExactBlockSums.
//                                 Three arrays of n doubles -- ratio then eta, log weight then weight, ln phi -- in LDS up to
//                                 kPsisLdsDraws draws beside the two selection arrays, in the workgroup's slice of the bounded
//                                 scratch beyond. No atomics, no inline assembly.
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_cov_exact.h"

namespace ppcx {

struct LooMmCovExactShared {
  double M[kCovNN], I[kCovNN], Minv[kCovNN];
  double b[kLooMmCovNc], zero[kLooMmCovNc], binv[kLooMmCovNc];
  double logJ;
};

template <bool LDS, bool SPLIT>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_cov_exact_kernel(LooMmThenArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmCovExactShared ms;
  const LooArgs& a = p.m.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_slice3(n));
  double* W = m.V + n;                                   // [n] log weights, then weights (m.V: [n] the ratios)
  double* LP = W + n;                                    // [n] ln phi
  double* E = m.V;                                       // [n] eta, once the ratios are dead
  const LooCell c = loo_cell<false>(a);
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  const bool excluded = c.excluded;
  double* o = p.out + (long)cell * loo_mm_cov_exact_fields(C);
  const double* rec = p.m.out + (long)cell * loo_mm_cov_fields(C);
  const bool matched = rec[5] > 0.0;                     // uniform: every thread reads the same word
  double* ks = o + kLooExactFields + 3;                  // khat_split
  if (tid == 0) loo_mm_cov_exact_store_state(o, C, rec);
  // ---- a cell that was not matched: ppcx_loo_exact_kernel's cell
  if (!matched) { loo_exact_cell<false, false>(a, c, m, nullptr, nullptr, p.log_tc, p.p_lo, p.p_hi, o, sh); return; }
  auto all_nan = [&]() { if (tid == 0) loo_exact_store_nan(o, y, excluded); };
  // ---- the states
  {
    const double* M = rec + kLooMmCovHead;
    const double* inv = p.m.inv + (long)cell * loo_mm_cov_inv_fields(C);
    for (int j = tid; j < nc * nc; j += kBlockThreads) {
      ms.M[j] = M[j]; ms.I[j] = j / nc == j % nc ? 1.0 : 0.0;
      if constexpr (SPLIT) ms.Minv[j] = inv[j];
    }
    if (tid < nc) {
      ms.b[tid] = M[nc * nc + tid]; ms.zero[tid] = 0.0;
      if constexpr (SPLIT) ms.binv[tid] = inv[nc * nc + tid];
    }
    if constexpr (SPLIT) if (tid == 0) ms.logJ = inv[nc * nc + nc];
  }
  __syncthreads();
  const LooMmGene g = loo_mm_gene(p.m, gi);
  const long h = SPLIT ? loo_mm_split_half(n) : n;       // the draws below h are transformed
  // ---- the ratios under the state(s), their tail and the normalised weights
  CountedRatios cr;
  if constexpr (!SPLIT) {
    cr = loo_mm_count_ratios(n, m.V, sh, [&](long i) {
      return loo_mm_cov_exact_ratio(g, i, LooMmAffine{ms.M, ms.b}, LooMmAffine{ms.I, ms.zero}, s);
    });
  } else {
    const double logJ = ms.logJ;
    cr = loo_mm_count_ratios(n, m.V, sh, [&](long i) {
      const bool first = i < h;
      const double* Mx = first ? ms.M : ms.I;
      const double* bx = first ? ms.b : ms.zero;
      const double* Mi = first ? ms.I : ms.Minv;
      const double* bi = first ? ms.zero : ms.binv;
      double lx;
      return loo_mm_split_ratio(g, i, LooMmAffine{Mx, bx}, LooMmAffine{Mi, bi}, logJ, s, &lx);
    });
  }
  if (cr.N == 0) { all_nan(); return; }
  const int M = psis_tail_len(cr.N, a.r_eff ? a.r_eff[cell] : 1.0);
  const LooTail lt = loo_cell_tail(m.V, n, cr.N, M, m.K, m.X, a.sel_pad, sh);
  loo_cell_lw<true>(m.V, W, n, cr.rmax, lt, M, m.K, sh);
  __syncthreads();                                       // no thread reads a ratio any more: V becomes E
  // ---- (eta, ln phi) at the proposal points
  const bool inval = loo_fill_eta_lnphi(n, p.log_tc, E, LP, [&](long i, double* sg) {
    const bool first = i < h;
    return loo_mm_cov_exact_eta(g, s, i, LooMmAffine{first ? ms.M : ms.I, first ? ms.b : ms.zero}, sg);
  });
  if (inval) { all_nan(); return; }
  // ---- the moments, the two tails at y, the interval (ppc_exact_sweeps); khat beside its nine fields
  const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, y, excluded, 1, p.p_lo, p.p_hi, tid == 0, o);
  if (tid == 0) {
    if constexpr (SPLIT) { o[kPpcExactFields] = ok ? rec[3] : NAN; *ks = ok ? lt.khat : NAN; }
    else o[kPpcExactFields] = ok ? lt.khat : NAN;
  }
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_cov_exact_kernel);

// the matching with the covariance step ahead of the kernel: its non-split instantiation (the elpd split is not needed), with
// the accumulated inverse as the second record
struct LooMmCovMatching {
  int fields(int C) const { return loo_mm_cov_fields(C); }
  int second(int C) const { return loo_mm_cov_inv_fields(C); }
  hipError_t launch(const LooMmArgs& q, const CellLaunch& c, hipStream_t st) const { return launch_loo_mm_cov_kernels(q, c, false, st); }
};

hipError_t loo_mm_cov_exact_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool split, double tc, double p_lo, double p_hi,
                                      double* out, size_t scratch_bytes, hipStream_t st) {
  return loo_mm_then_fit_cells(fc, LooMmCovMatching{}, k_threshold, max_iters, tc, p_lo, p_hi, loo_mm_cov_exact_fields(fc.d.C), out,
                               scratch_bytes, st, [=](bool lds) { return pick_kernel<ppcx_loo_mm_cov_exact_kernel_of>(lds, split); });
}

}  // namespace ppcx
