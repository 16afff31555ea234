// ppcx_loo_exact.h -- the exact leave-one-out predictive tail probabilities and interval of a cell (ppcx_fit_loo_predict_exact,
// ppcx_fit_loo_predict_exact_approx): the Rao-Blackwellised form of ppcx_loo_predict.h. Given draw i, the count of cell (g, s) is
// negative binomial with mean mu_i = e^{eta_i} and size phi_i; the leave-one-out predictive distribution of the cell is the
// mixture of those n negative binomials under the PSIS weights w_i of the cell, and its cdf the weighted average of their cdfs
// (ppcx_nbcdf.h). No predictive count is drawn, so a tail probability that PSIS rests on a few heavy draws is not decided by
// as many sampled integers. In R this is loo::E_loo on the draws' exact cdfs; no function of loo or bayesplot does it.
// Restated from the published definitions (Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024; Magnusson et al. 2019 for the
// approximate posterior); not run against R.
//
// Shared by the gfx950 kernel (ppcx_loo_exact.hip) and the CPU check (tests/loo_exact_host): the blocks below are
// `__host__ __device__`; loo_exact_cell_host at the end is their sequential composition.
//
// One cell from its count y, whether the model excludes it, r_eff and, per draw i = 0 .. n - 1, its linear predictor eta_i,
// sigma_raw_i and its log-likelihood ll_i (a fit: loo_ll(y, eta_i, sigma_raw_i), the model's phi = exp(-sigma_raw_i) without the
// truncation compensation); an ADVI fit also a_i = log_p_i - log_g_i:
//   0. ln phi_i = ln(truncation_compensation) - sigma_raw_i, phi_i = exp(ln phi_i), mu_i = exp(eta_i): ppcx_ppc_exact.h step 0.
//      Every statistic of the cell is NaN (y and excluded are still reported) where a draw has invalid parameters
//      (ppc_exact_invalid), where a continued fraction reaches its cap, or where the ratios are NaN: ppcx_loo_predict.h step 1
//      (a NaN ratio; +Inf where the cell is not excluded; no participating draw), ppcx_loo_ap.h step 0 for an ADVI fit.
//   1. The weights w_i and khat as ppcx_fit_loo_predict forms them: ratios r_i = -ll_i (an ADVI fit: a_i - ll_i), the tail of
//      psis_tail_len(N, r_eff) draws, the log weight of draw i by loo_predict_lw at its tail position under the TIE RULE of
//      ppcx_loo_predict.h step 2, w_i = exp(lw_i - max lw) / sum. A draw whose ratio is -Inf has weight 0.
//   2. mean = sum_i w_i mu_i;  sd = sqrt(sum_i w_i (mu_i + mu_i^2 / phi_i) + sum_i w_i (mu_i - mean)^2) (ppc_exact_var_terms).
//   3. p_le = sum_i w_i P_i(X <= y),  p_ge = sum_i w_i P_i(X >= y): nb2_log_tails_ln per draw, each from its own sum.
//   4. L = sum_i w_i P_i(X <= k), U = sum_i w_i P_i(X > k) (nb2_cdf_pair); F(k) = L where L <= U, else 1 - U;
//      lower, upper = Q(p_lo), Q(p_hi) by ppc_exact_bracket(mean, sd, ..) and ppc_exact_quantile, the search of ppcx_ppc_exact.h.
//   5. A cell the model excludes. A NUTS fit has already held it out: the weight of every draw is 1 and every sum is divided
//      by n -- the blocks of ppcx_ppc_exact.h themselves, so the first nine fields are ppcx_fit_ppc_exact's bit for bit --
//      and khat = NaN. An ADVI fit: weighted by a_i alone, khat the overall k-hat (ppcx_loo_ap.h).
//      Both forms are ONE composition: every sum is sum_i w_i f_i, divided by `den` -- n with w_i = 1 for the uniform cell, 1 with
//      the normalised weights otherwise (a product with 1 and a quotient by 1 are exact): ppc_exact_sweeps of ppcx_ppc_exact.h,
//      which this header and that one both call.
//   6. The fields: mean, sd, p_le, p_ge, lower, upper, y, excluded, outside as ppc_exact_store / ppc_exact_store_nan lay them
//      out, then khat.
// Every sum runs in a fixed order with contraction off: a cell's fields are a function of its own draws only.
#pragma once
#include <stdint.h>
#include "ppcx_loo_ap.h"
#include "ppcx_ppc_exact.h"

namespace ppcx {

constexpr int kLooExactFields = 10;            // kPpcExactFields, then khat (include/ppcx.h PPCX_LOO_EXACT_FIELDS)

// step 6: the tenth field beside ppc_exact_sweeps' nine
PPCX_HD void loo_exact_store_nan(double* o, int y, bool excluded) {
  ppc_exact_store_nan(o, y, excluded);
  o[kPpcExactFields] = NAN;
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
namespace ppcx {
// Step 1 for one cell, sequentially, from its ratios r[0 .. n) (none NaN or +Inf, not all -Inf): the log weight of every draw
// in draw order (-Inf for a draw that takes no part) and k-hat. loo_ap_weights_host's composition with r_eff.
inline void loo_exact_log_weights_host(const double* r, long n, double r_eff, std::vector<double>& lw, double* khat_out) {
  std::vector<long> ix;
  for (long i = 0; i < n; ++i) if (r[i] != -INFINITY) ix.push_back(i);
  const long N = (long)ix.size();
  std::stable_sort(ix.begin(), ix.end(), [&](long p, long q) { return r[p] < r[q]; });
  std::vector<double> rs(N);
  for (long i = 0; i < N; ++i) rs[i] = r[ix[i]];
  const double mx = rs[N - 1];
  const int M = psis_tail_len(N, r_eff);
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
}
// the whole spec for one cell, sequentially, for the CPU check: out[kLooExactFields]. a: the log ratios of an ADVI fit, or null
// (a NUTS fit). max_iters (may be null): the largest number of continued-fraction steps any evaluation took.
inline void loo_exact_cell_host(const double* ll, const double* eta, const double* sigma_raw, const double* a, long n, int y,
                                bool excluded, double r_eff, double tc, double p_lo, double p_hi, double* out,
                                int* max_iters = nullptr) {
  PPCX_NO_CONTRACT
  const double log_tc = log(tc);
  int mx = 0;
  if (max_iters) *max_iters = 0;
  auto lnphi = [&](long i) { return ppc_exact_lnphi(sigma_raw[i], log_tc); };
  // ---- step 0, the ratios
  std::vector<double> r((size_t)n);
  long N = 0;
  for (long i = 0; i < n; ++i) {
    r[i] = a ? loo_ap_ratio(a[i], ll[i], excluded) : -ll[i];
    const bool bad = a ? loo_ap_bad(a[i], ll[i], r[i], excluded) : isnan(r[i]) || (!excluded && r[i] == INFINITY);
    if (bad) { loo_exact_store_nan(out, y, excluded); return; }
    N += r[i] != -INFINITY;
  }
  const bool uniform = !a && excluded;
  if (!uniform && N == 0) { loo_exact_store_nan(out, y, excluded); return; }
  for (long i = 0; i < n; ++i)
    if (ppc_exact_invalid(eta[i], ppc_exact_phi(lnphi(i)))) { loo_exact_store_nan(out, y, excluded); return; }
  // ---- step 1 (step 5: the uniform cell)
  std::vector<double> w((size_t)n, 1.0);
  double khat = NAN;
  const long den = uniform ? n : 1;
  if (!uniform) {
    loo_exact_log_weights_host(r.data(), n, a ? 1.0 : r_eff, w, &khat);
    double mxw = -INFINITY, sw = 0.0;
    for (long i = 0; i < n; ++i) mxw = w[i] > mxw ? w[i] : mxw;
    for (long i = 0; i < n; ++i) { w[i] = exp(w[i] - mxw); sw += w[i]; }
    for (long i = 0; i < n; ++i) w[i] = w[i] / sw;
  }
  // ---- steps 2 - 6
  const bool ok = ppc_exact_sweeps(ExactHostSums{w.data(), eta, sigma_raw, log_tc, n, &mx}, y, excluded, den, p_lo, p_hi, true, out);
  out[kPpcExactFields] = ok ? khat : NAN;
  if (max_iters) *max_iters = mx;
}
}  // namespace ppcx
#endif
