// ppcx_loo_mm_split.h -- the split transformation of gene-local moment matching (ppcx_fit_loo_moment_match_split,
// ppcx_fit_loo_predict_exact_moment_match_split): section 4 of Paananen, Piironen, Buerkner, Vehtari (2021), "Implicitly adaptive
// importance sampling" (loo:::loo_moment_match_split, what loo::loo_moment_match(split = TRUE) runs), restated for the
// coordinates of ONE gene as ppcx_loo_mm.h restates the matching. Restated from the paper and the published package; not run
// against R.
//
// Why. The matched draws t_i = A theta_i + B of ppcx_loo_mm.h are no longer a sample of a known density: A and B were computed
// from the draws themselves, so the matched estimate is biased and a matched khat is necessary, not sufficient. The split
// estimator transforms only HALF the draws, keeps the other half, and weights all of them against the two-component mixture
// they really come from -- the posterior p and its image under T, p(T^-1 x) / |J| -- so the estimate is consistent whatever the
// matching did. loo needs log_prob at T(theta) and T^-1(theta); here the terms of the log posterior outside the gene are the
// same in both components and cancel draw by draw, so the local density q of ppcx_loo_mm.h at three states -- the match, the
// identity and the inverse -- is enough and neither log_prob nor lp__ is needed.
//
// Shared by the gfx950 kernel (ppcx_loo_mm_split.hip) and the CPU check (tests/loo_mm_split_twin): the blocks below are
// `__host__ __device__`; loo_mm_split_cell_host and loo_mm_exact_split_cell_host at the end are their sequential compositions.
//
// One cell (g, s) from what ppcx_loo_mm.h reads and the record it leaves for the cell (khat, khat_before, iterations, scale A,
// shift B):
//   1. iterations == 0: nothing is split. The record is copied bit for bit, elpd_loo_matched = elpd_loo, khat_split = NaN. The
//      predictive form: ppcx_loo_exact.h itself, the same blocks in the same order as the unmatched path of ppcx_loo_mm_exact.h,
//      so the ten fields are ppcx_fit_loo_predict_exact's bits.
//   2. iterations > 0: with n draws in the fit's order, h = n / 2 (integer division). The inverse state per coordinate c of the
//      gene: Ainv_c = 1 / A_c, Binv_c = -(B_c / A_c); a row that is no coordinate of the gene (loo_mm_is_coord false) keeps (1, 0).
//      logJ = sum log A_c over the gene's coordinates in ascending row order.
//   3. Draw i < h: the proposal point is x_i = A theta_i + B; qx and ll_x by loo_mm_density at (A, B), qinv by it at the identity.
//   4. Draw i >= h: the proposal point is x_i = theta_i; qx and ll_x by loo_mm_density at the identity, qinv by it at (Ainv, Binv).
//   5. With d = qinv - logJ the log ratio is r_i = qx - ll_x - logaddexp(qx, d), logaddexp(a, b) = max(a, b) + log1p(exp(-|a - b|));
//      a value that is not finite becomes -Inf (the draw takes no part). loo's lwi_half.
//   6. PSIS on r exactly as ppcx_loo_mm.h step 3 runs it on a candidate (the tail length from the participating draws and the same
//      r_eff, the tie rule, the smoothing order): the log weights lw and khat_split. No participating draw: the cell's statistics
//      are NaN.
//   7. elpd_loo = logsumexp(lw + ll_x) - logsumexp(lw); p_loo = lpd - elpd_loo with lpd that of the original draws; looic =
//      -2 elpd_loo. khat stays the matching's final k, as loo reports it; khat_before, iterations, scale and shift are the
//      matching's bits. Appended: elpd_loo_matched (the unsplit estimate of ppcx_loo_mm.h), khat_split.
//   8. The predictive under these weights: w_i = exp(lw_i - max lw) / sum (ppcx_loo_exact.h step 1); eta_i and sigma_raw_i at x_i,
//      the transformed draw in the first half and the original draw in the second; ppc_exact_sweeps with den = 1. An invalid x_i
//      (ppc_exact_invalid) makes the cell's statistics NaN, khat and khat_split included. Otherwise khat is the matching's final
//      k; khat_split is appended behind the record of ppcx_loo_mm_exact.h.
//   9. The first half is the first h draws in the fit's order, i.e. whole leading chains (and the leading part of the middle one
//      when the chain count is odd), as loo takes them.
//  10. Every sum runs in a fixed order with contraction off: a cell's fields depend on its own gene's data only.
// Left out: the covariance step (ppcx_loo_mm_cov.h runs steps 2 - 7 on its affine map, ppcx_loo_mm_cov_exact.h step 8), mcse / n_eff of a
// matched cell, ADVI fits. khat_split is a diagnostic of the split ratios, not
// a gate: nothing is refused or repeated on its account.
#pragma once
#include <stdint.h>
#include "ppcx_loo_mm.h"
#include "ppcx_loo_mm_exact.h"

namespace ppcx {

PPCX_HD int loo_mm_split_fields(int C) { return loo_mm_fields(C) + 2; }               // PPCX_LOO_MM_SPLIT_FIELDS(C)
PPCX_HD int loo_mm_exact_split_fields(int C) { return loo_mm_exact_fields(C) + 1; }   // PPCX_LOO_MM_EXACT_SPLIT_FIELDS(C)

// step 2: the half, the inverse state of row c and the log Jacobian of the state A[C + 1]
PPCX_HD long loo_mm_split_half(long n) { return n / 2; }
PPCX_HD double loo_mm_split_Ainv(const LooMmGene& g, int c, const double* A) { return loo_mm_is_coord(g, c) ? 1.0 / A[c] : 1.0; }
PPCX_HD double loo_mm_split_Binv(const LooMmGene& g, int c, const double* A, const double* B) {
  return loo_mm_is_coord(g, c) ? -(B[c] / A[c]) : 0.0;
}
PPCX_HD double loo_mm_split_logJ(const LooMmGene& g, const double* A) {
  PPCX_NO_CONTRACT
  double lj = 0.0;
  for (int c = 0; c <= g.C; ++c) if (loo_mm_is_coord(g, c)) lj += log(A[c]);
  return lj;
}
// step 5
PPCX_HD double loo_mm_split_logaddexp(double a, double b) {
  PPCX_NO_CONTRACT
  const double mx = a > b ? a : b;
  return mx + log1p(exp(-fabs(a - b)));
}
// steps 3 - 5: the ratio of draw i, whose proposal point lies under the state x and whose other mixture component is
// evaluated under the state inv; *ll_x the log-likelihood of the cell of sample s at the proposal point
template <class State>
PPCX_HD double loo_mm_split_ratio(const LooMmGene& g, long i, const State& x, const State& inv, double logJ, int s, double* ll_x) {
  PPCX_NO_CONTRACT
  double l, li;
  const double qx = loo_mm_density(g, i, x, s, &l);
  const double qinv = loo_mm_density(g, i, inv, s, &li);
  const double d = qinv - logJ;
  const double r = qx - l - loo_mm_split_logaddexp(qx, d);
  *ll_x = l;
  return isfinite(r) ? r : -INFINITY;
}
// the same under diagonal states (Ax, Bx) and (Ai, Bi) given by their arrays
PPCX_HD double loo_mm_split_ratio(const LooMmGene& g, long i, const double* Ax, const double* Bx, const double* Ai, const double* Bi,
                                  double logJ, int s, double* ll_x) {
  return loo_mm_split_ratio(g, i, LooMmDiag{Ax, Bx}, LooMmDiag{Ai, Bi}, logJ, s, ll_x);
}
// step 7: the record of ppcx_loo_mm.h, then elpd_loo_matched and khat_split (NaN until a cell is split)
PPCX_HD void loo_mm_split_store_record(double* o, int C, const double* rec) {
  const int f = loo_mm_fields(C);
  for (int c = 0; c < f; ++c) o[c] = rec[c];
  o[f] = rec[0]; o[f + 1] = NAN;
}
PPCX_HD void loo_mm_split_store(double* o, int C, double elpd, double lpd, double khat_split) {
  PPCX_NO_CONTRACT
  o[0] = elpd; o[1] = lpd - elpd; o[2] = -2.0 * elpd; o[loo_mm_fields(C) + 1] = khat_split;
}
PPCX_HD void loo_mm_split_store_nan(double* o, int C) { o[0] = o[1] = o[2] = NAN; o[loo_mm_fields(C) + 1] = NAN; }

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
namespace ppcx {
// steps 2 - 6 for one cell, sequentially: the ratios' log weights lw [n] and ll_x [n]; returns khat_split, *any whether a draw
// takes part. A, B: the record's state [C + 1]
inline double loo_mm_split_weights_host(const LooMmGene& g, int s, double r_eff, const double* A, const double* B, std::vector<double>& lw,
                                        std::vector<double>& lx, bool* any) {
  const long n = g.n, h = loo_mm_split_half(n);
  const int nc = g.C + 1;
  const std::vector<double> one((size_t)nc, 1.0), zero((size_t)nc, 0.0);
  std::vector<double> Ainv((size_t)nc), Binv((size_t)nc), r((size_t)n);
  for (int c = 0; c < nc; ++c) { Ainv[c] = loo_mm_split_Ainv(g, c, A); Binv[c] = loo_mm_split_Binv(g, c, A, B); }
  const double logJ = loo_mm_split_logJ(g, A);
  lx.assign((size_t)n, 0.0);
  *any = false;
  for (long i = 0; i < n; ++i) {
    const bool first = i < h;
    r[i] = loo_mm_split_ratio(g, i, first ? A : one.data(), first ? B : zero.data(), first ? one.data() : Ainv.data(),
                              first ? zero.data() : Binv.data(), logJ, s, &lx[i]);
    *any = *any || r[i] != -INFINITY;
  }
  return loo_mm_psis_host(r, r_eff, lw);
}
// the elpd form from a record rec[loo_mm_fields(C)] of ppcx_loo_mm.h: out[loo_mm_split_fields(C)]
inline void loo_mm_split_from_record_host(const LooMmGene& g, int s, double r_eff, const double* rec, double* out) {
  PPCX_NO_CONTRACT
  const long n = g.n;
  const int C = g.C, nc = C + 1;
  loo_mm_split_store_record(out, C, rec);
  if (!(rec[5] > 0.0)) return;
  const double* A = rec + kLooMmHead;
  const double* B = A + nc;
  // lpd of the original draws, as loo_mm_cell_host forms it
  const std::vector<double> one((size_t)nc, 1.0), zero((size_t)nc, 0.0);
  std::vector<double> ll((size_t)n);
  for (long i = 0; i < n; ++i) ll[i] = loo_mm_cell_ll(g, i, one.data(), zero.data(), s);
  double lpd;
  loo_mm_lpd_host(ll, &lpd);
  std::vector<double> lw, lx;
  bool any;
  const double khat_split = loo_mm_split_weights_host(g, s, r_eff, A, B, lw, lx, &any);
  if (!any) { loo_mm_split_store_nan(out, C); return; }
  std::vector<double> a, b;
  for (long i = 0; i < n; ++i) if (lw[i] != -INFINITY) { a.push_back(lw[i] + lx[i]); b.push_back(lw[i]); }
  loo_mm_split_store(out, C, loo_logsumexp_host(a) - loo_logsumexp_host(b), lpd, khat_split);
}
// the predictive form from the same record: out[loo_mm_exact_split_fields(C)]
inline void loo_mm_exact_split_from_record_host(const LooMmGene& g, int s, double r_eff, double tc, double p_lo, double p_hi,
                                                const double* rec, double* out) {
  const long h = loo_mm_split_half(g.n);
  const int C = g.C, nc = C + 1;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  double* ks = out + loo_mm_exact_fields(C);
  loo_mm_exact_store_state(out, C, rec);
  *ks = NAN;
  // ---- step 1
  if (!(rec[5] > 0.0)) { loo_mm_exact_unmatched_host(g, s, r_eff, tc, p_lo, p_hi, out); return; }
  // ---- steps 2 - 6
  const std::vector<double> one((size_t)nc, 1.0), zero((size_t)nc, 0.0);
  const double* A = rec + kLooMmHead;
  const double* B = A + nc;
  std::vector<double> w, lx;
  bool any;
  const double khat_split = loo_mm_split_weights_host(g, s, r_eff, A, B, w, lx, &any);
  if (!any) { loo_exact_store_nan(out, y, excluded); return; }
  // ---- step 8
  loo_mm_normalise_host(w);
  const bool ok = loo_mm_predictive_host(g, s, w, tc, p_lo, p_hi, out, [&](long i, const double** a, const double** b) {
    *a = i < h ? A : one.data(); *b = i < h ? B : zero.data();
  });
  out[kPpcExactFields] = ok ? rec[3] : NAN;
  *ks = ok ? khat_split : NAN;
}
// the whole spec for one cell, sequentially, for the CPU check: the matching of ppcx_loo_mm.h, then the split
inline void loo_mm_split_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, double* out) {
  std::vector<double> rec((size_t)loo_mm_fields(g.C));
  loo_mm_cell_host(g, s, r_eff, k_threshold, max_iters, rec.data());
  loo_mm_split_from_record_host(g, s, r_eff, rec.data(), out);
}
inline void loo_mm_exact_split_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, double tc, double p_lo,
                                         double p_hi, double* out) {
  std::vector<double> rec((size_t)loo_mm_fields(g.C));
  loo_mm_cell_host(g, s, r_eff, k_threshold, max_iters, rec.data());
  loo_mm_exact_split_from_record_host(g, s, r_eff, tc, p_lo, p_hi, rec.data(), out);
}
}  // namespace ppcx
#endif
