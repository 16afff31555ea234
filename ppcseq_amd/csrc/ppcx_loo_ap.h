// ppcx_loo_ap.h -- PSIS-LOO per observed cell of an ADVI fit (ppcx_fit_loo_approx, ppcx_fit_loo_predict_approx): what
// loo::loo_approximate_posterior(log_lik, log_p, log_g) reports per observation, and loo::E_loo with its weights. Magnusson,
// Andersen, Jonasson, Vehtari (2019), "Bayesian leave-one-out cross-validation for large data", section 3.1: the draws come
// from the approximation g, not from the posterior p, so the importance ratio of draw i for cell c carries the correction
// p / g of the draw as well as the cell's own 1 / likelihood. The tail fit is ppcx_psis.h's, the smoothing ppcx_loo.h's.
// Restated from the published package and its paper; not run against R.
//
// Shared by the gfx950 kernels (ppcx_loo.hip, ppcx_loo_predict.hip) and the CPU check (tests/loo_ap_host): the blocks below are
// `__host__ __device__`; loo_ap_cell_host at the end is their sequential composition.
//
// One cell from its column ll[0 .. n) (ppcx_loo.h) and the fit's log ratios a[0 .. n), a_i = log_p_i - log_g_i (the array
// ppcx_fit_psis runs on: -Inf where log_p or log_g is not finite):
//   0. r_i = a_i - ll_i, one rounded subtraction (loo adds log_p - log_g to -log_lik). A NaN in a_i or ll_i, or r_i = +Inf:
//      every field NaN. A draw with r_i = -Inf takes no part; N = the other draws. N = 0: every field NaN.
//   1 - 3. ppcx_loo.h steps 1 - 3 on these ratios with r_eff = 1: M = ceil(min(0.2 N, 3 sqrt N)), the shift by the largest
//      ratio, k-hat, the smoothed tail, the truncation at 0. Tied ratios may now have different ll, so the TIE RULE of
//      ppcx_loo_predict.h step 2 holds: a stable sort, tied draws in draw order; a draw's log weight is loo_predict_lw at its
//      tail position (loo_predict_tail_pos).
//   4. elpd_loo = logsumexp(lw + ll) - logsumexp(lw); lpd = logsumexp(ll) - log N, unweighted, over the draws that take part
//      (loo's pointwise lpd for an approximate posterior as well); p_loo = lpd - elpd_loo; looic = -2 elpd_loo; khat = k-hat.
// A cell the model excludes is already held out of p, but the draws still come from g: r_i = a_i alone (ll = +Inf would leave
// the sums undefined: every field NaN), elpd_loo by the same formula with those weights, p_loo = 0, looic = -2 elpd_loo, and
// khat the k-hat of a -- the overall k-hat of ppcx_fit_psis (column -1), the same for every excluded cell.
// The predictive interval and LOO-PIT (ppcx_fit_loo_predict_approx): the normalised weights of step 3, those of an excluded
// cell included, take the place of the NUTS weights in ppcx_loo_predict.h step 3; an excluded cell has no uniform path.
// The Monte-Carlo standard error and n_eff (ppcx_loo.h steps 5 - 8) are not defined here for these weights.
// Every reduction runs in a fixed order: a cell's fields depend on its own column and on a only.
#pragma once
#include "ppcx_loo_predict.h"

namespace ppcx {

// step 0: the ratio of a draw
PPCX_HD double loo_ap_ratio(double a, double ll, bool excluded) {
  PPCX_NO_CONTRACT
  return excluded ? a : a - ll;
}
// whether the draw makes the whole cell NaN
PPCX_HD bool loo_ap_bad(double a, double ll, double r, bool excluded) {
  return isnan(a) || isnan(ll) || r == INFINITY || (excluded && ll == INFINITY);
}
// logsumexp from the maximum and the sum of exp(v - max) (-Inf where every term is -Inf)
PPCX_HD double loo_ap_lse(double mx, double sum) { return mx == -INFINITY ? -INFINITY : mx + log(sum); }

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
namespace ppcx {
// Steps 0 - 3 for one cell, sequentially: the ratio and the log weight of every draw in draw order (both -Inf for a draw that
// takes no part) and k-hat. Returns false where the cell is NaN.
inline bool loo_ap_weights_host(const double* ll, const double* a, long n, bool excluded, std::vector<double>& r,
                                std::vector<double>& lw, double* khat_out) {
  r.assign((size_t)n, 0.0);
  std::vector<long> ix;                                  // the participating draws
  for (long i = 0; i < n; ++i) {
    r[i] = loo_ap_ratio(a[i], ll[i], excluded);
    if (loo_ap_bad(a[i], ll[i], r[i], excluded)) return false;
    if (r[i] != -INFINITY) ix.push_back(i);
  }
  const long N = (long)ix.size();
  if (N == 0) return false;
  std::stable_sort(ix.begin(), ix.end(), [&](long p, long q) { return r[p] < r[q]; });
  std::vector<double> rs(N);
  for (long i = 0; i < N; ++i) rs[i] = r[ix[i]];
  const double mx = rs[N - 1];
  const int M = psis_tail_len(N);
  double khat = INFINITY, sigma = 0.0, ec = 0.0;
  bool smooth = false;
  if (M >= 5 && M < N && rs[N - M] != mx) {
    const PsisTailHost t = psis_tail_host(rs.data(), N, M);
    sigma = -t.k_mean / t.theta_hat; ec = t.ec;
    khat = psis_adjust(t.k_mean, M);
    smooth = loo_smooth_ok(khat, sigma);
  }
  lw.assign((size_t)n, -INFINITY);
  for (long i = 0; i < N; ++i) {
    const long pos = i - (N - M) + 1;                    // tail position 1 .. M of the i-th smallest
    lw[ix[i]] = loo_predict_lw(rs[i], mx, smooth && pos > 0 ? (int)pos : 0, M, khat, sigma, ec);
  }
  *khat_out = khat;
  return true;
}
// the whole spec for one cell, sequentially, for the CPU check: out[kLooFields]
inline void loo_ap_cell_host(const double* ll, const double* a, long n, bool excluded, double* out) {
  std::vector<double> r, lw;
  double khat;
  if (!loo_ap_weights_host(ll, a, n, excluded, r, lw, &khat)) { out[0] = out[1] = out[2] = out[3] = NAN; return; }
  std::vector<double> w, wl, l;
  for (long i = 0; i < n; ++i)
    if (r[i] != -INFINITY) { w.push_back(lw[i]); wl.push_back(lw[i] + ll[i]); l.push_back(ll[i]); }
  const double elpd = loo_logsumexp_host(wl) - loo_logsumexp_host(w);
  const double lpd = loo_logsumexp_host(l) - log((double)l.size());
  out[0] = elpd; out[1] = excluded ? 0.0 : lpd - elpd; out[2] = -2.0 * elpd; out[3] = khat;
}
}  // namespace ppcx
#endif
