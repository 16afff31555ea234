// ppcx_loo_mm_cov_exact.h -- the exact leave-one-out predictive tails and interval of a cell under the weights of the matching
// with the covariance step (ppcx_fit_loo_predict_exact_moment_match_cov): ppcx_loo_exact.h for the cells that ppcx_loo_mm_cov.h
// has matched, optionally under its split transformation. ppcx_loo_mm_exact.h and ppcx_loo_mm_split.h step 8 are the same
// statistic under the per-coordinate state; here the state is the affine map (M, b) and the point of a draw is M theta + b.
// Restated from Paananen et al. (2021); not run against R.
//
// Shared by the gfx950 kernel (ppcx_loo_mm_cov_exact.hip) and the CPU check (tests/loo_mm_cov_exact_cpu): the blocks below are
// `__host__ __device__`; loo_mm_cov_exact_cell_host at the end is their sequential composition.
//
// One cell (g, s) of a checked gene from what ppcx_loo_mm_cov.h reads and the record it leaves for the cell (khat, khat_before,
// iterations, cov_iterations, M, b) and, for the split, the accumulated inverse (Minv, binv, logJ) of its step 6 -- the
// accumulated one, which is the definition, not an inverse taken from the final M:
//   1. iterations == 0 (a cell that is excluded, NaN, at or below the threshold, run with max_iters = 0, or without an accepted
//      candidate): ppcx_loo_exact.h itself -- the same blocks in the same order as the unmatched path of ppcx_loo_mm_exact.h, so
//      the ten fields are ppcx_fit_loo_predict_exact's bit for bit. The affine path is NOT evaluated at the identity for these
//      cells.
//   2. iterations > 0, unsplit, the weights: r_i = loo_mm_ratio(q(t_i; h_i), Q0_i, ll_gs(t_i)), q by loo_mm_density under
//      LooMmAffine at (M, b) and Q0_i by it under LooMmAffine at the identity -- as ppcx_loo_mm_cov_kernel forms Q0 -- in the same
//      visit of draw i. These are the ratios of the candidate that the matching accepted last, so khat is its final khat bit
//      for bit. PSIS on r as ppcx_loo_mm.h step 3 runs it; w_i = exp(lw_i - max lw) / sum as ppcx_loo_exact.h step 1.
//   3. iterations > 0, split, the weights: steps 2 - 6 of ppcx_loo_mm_split.h on the three states (M, b), the identity and
//      (Minv, binv) with the accumulated logJ: exactly the ratio sweep of ppcx_loo_mm_cov.h step 7. khat stays the matching's;
//      khat_split is reported. No participating draw: the cell's record is NaN, khat and khat_split included.
//   4. The predictive at the proposal points: the point t = M theta_i + b is formed once per draw (unsplit: every draw; split:
//      i < n / 2, the original draw -- the point under the identity state -- from there on); eta_i = loo_mm_eta_at(.., t),
//      sigma_raw_i = t(C), ln phi_i = ppc_exact_lnphi(sigma_raw_i, ln tc); ppc_exact_sweeps over (w, eta, ln phi) with den = 1. A
//      proposal point with invalid parameters (ppc_exact_invalid) makes the cell's statistics NaN, khat (and khat_split) included.
//   5. The record, loo_mm_cov_exact_fields(C) = 14 + (C + 1)^2 + (C + 1): the ten fields of ppcx_loo_exact.h with khat the final
//      one, then khat_before, iterations, cov_iterations, khat_split (NaN without split or with iterations == 0), then
//      transform [C + 1][C + 1] row-major and shift [C + 1], the covariance record's bits.
// Left out: mcse / n_eff of a matched cell, ADVI fits. Every sum runs in a fixed order with contraction off: a cell's fields
// depend on its own gene's data only.
#pragma once
#include <stdint.h>
#include "ppcx_loo_mm_cov.h"
#include "ppcx_loo_mm_exact.h"

namespace ppcx {

constexpr int kLooMmCovExactHead = kLooExactFields + 4;   // ppcx_loo_exact.h's ten, khat_before, iterations, cov_iterations, khat_split
PPCX_HD int loo_mm_cov_exact_fields(int C) { return kLooMmCovExactHead + (C + 1) * (C + 1) + (C + 1); }   // PPCX_LOO_MM_COV_EXACT_FIELDS(C)
// what the matching leaves beside its record for the split: Minv [nc][nc], binv [nc], logJ
PPCX_HD int loo_mm_cov_inv_fields(int C) { return (C + 1) * (C + 1) + (C + 1) + 1; }

// step 2: the ratio of draw i under the state st; id: the identity state
PPCX_HD double loo_mm_cov_exact_ratio(const LooMmGene& g, long i, const LooMmAffine& st, const LooMmAffine& id, int s) {
  double l, l0;
  const double q = loo_mm_density(g, i, st, s, &l);
  const double q0 = loo_mm_density(g, i, id, s, &l0);
  return loo_mm_ratio(q, q0, l);
}
// step 4: the linear predictor and sigma_raw of the cell of sample s at the point of draw i under the state st
PPCX_HD double loo_mm_cov_exact_eta(const LooMmGene& g, int s, long i, const LooMmAffine& st, double* sigma_raw) {
  const LooMmAffine::Point t = st.point(g, i);
  *sigma_raw = t(g.C);
  return loo_mm_eta_at(g, s, t(0), t);
}
// step 5: the tail of a cell's record behind its ten fields, from the record rec[loo_mm_cov_fields(C)] of ppcx_loo_mm_cov.h
PPCX_HD void loo_mm_cov_exact_store_state(double* o, int C, const double* rec) {
  const int nc = C + 1;
  o[kLooExactFields] = rec[4]; o[kLooExactFields + 1] = rec[5]; o[kLooExactFields + 2] = rec[6]; o[kLooExactFields + 3] = NAN;
  for (int c = 0; c < nc * nc + nc; ++c) o[kLooMmCovExactHead + c] = rec[kLooMmCovHead + c];
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
namespace ppcx {
// step 4: the predictive under the normalised weights w at the states state(i) of every draw: the nine fields of
// ppc_exact_sweeps into out and true, or the cell's NaN record and false (an invalid point, a failed sweep)
template <class F>
inline bool loo_mm_cov_predictive_host(const LooMmGene& g, int s, const std::vector<double>& w, double tc, double p_lo, double p_hi,
                                       double* out, F state) {
  PPCX_NO_CONTRACT
  const long n = g.n;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  const double log_tc = log(tc);
  std::vector<double> eta((size_t)n), sg((size_t)n);
  for (long i = 0; i < n; ++i) {
    eta[i] = loo_mm_cov_exact_eta(g, s, i, state(i), &sg[i]);
    if (ppc_exact_invalid(eta[i], ppc_exact_phi(ppc_exact_lnphi(sg[i], log_tc)))) { loo_exact_store_nan(out, y, excluded); return false; }
  }
  int mx = 0;
  return ppc_exact_sweeps(ExactHostSums{w.data(), eta.data(), sg.data(), log_tc, n, &mx}, y, excluded, 1, p_lo, p_hi, true, out);
}
// the whole spec for one cell, sequentially, for the CPU check: out[loo_mm_cov_exact_fields(C)]
inline void loo_mm_cov_exact_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, bool split, double tc,
                                       double p_lo, double p_hi, double* out) {
  const long n = g.n;
  const int C = g.C, nc = C + 1;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  std::vector<double> rec((size_t)loo_mm_cov_fields(C)), inv((size_t)loo_mm_cov_inv_fields(C));
  loo_mm_cov_cell_host(g, s, r_eff, k_threshold, max_iters, false, rec.data(), nullptr, inv.data());
  loo_mm_cov_exact_store_state(out, C, rec.data());
  double* ks = out + kLooExactFields + 3;
  // ---- step 1
  if ((int)rec[5] == 0) { loo_mm_exact_unmatched_host(g, s, r_eff, tc, p_lo, p_hi, out); return; }
  std::vector<double> I((size_t)nc * nc), zero((size_t)nc);
  loo_mm_cov_identity(I.data(), zero.data(), nc);
  const double* M = rec.data() + kLooMmCovHead;
  const double* b = M + nc * nc;
  const LooMmAffine fwd{M, b}, id{I.data(), zero.data()}, back{inv.data(), inv.data() + nc * nc};
  std::vector<double> r((size_t)n), w;
  if (!split) {
    // ---- step 2
    for (long i = 0; i < n; ++i) r[i] = loo_mm_cov_exact_ratio(g, i, fwd, id, s);
    const double khat = loo_mm_psis_host(r, r_eff, w);
    if (!loo_mm_normalise_host(w)) { loo_exact_store_nan(out, y, excluded); return; }
    const bool ok = loo_mm_cov_predictive_host(g, s, w, tc, p_lo, p_hi, out, [&](long) { return fwd; });
    out[kPpcExactFields] = ok ? khat : NAN;
    return;
  }
  // ---- step 3
  const long h = loo_mm_split_half(n);
  const double logJ = inv[(size_t)nc * nc + nc];
  bool any = false;
  for (long i = 0; i < n; ++i) {
    double lx;
    r[i] = i < h ? loo_mm_split_ratio(g, i, fwd, id, logJ, s, &lx) : loo_mm_split_ratio(g, i, id, back, logJ, s, &lx);
    any = any || r[i] != -INFINITY;
  }
  const double khat_split = loo_mm_psis_host(r, r_eff, w);
  if (!any) { loo_exact_store_nan(out, y, excluded); return; }
  loo_mm_normalise_host(w);
  const bool ok = loo_mm_cov_predictive_host(g, s, w, tc, p_lo, p_hi, out, [&](long i) { return i < h ? fwd : id; });
  out[kPpcExactFields] = ok ? rec[3] : NAN;
  *ks = ok ? khat_split : NAN;
}
}  // namespace ppcx
#endif
