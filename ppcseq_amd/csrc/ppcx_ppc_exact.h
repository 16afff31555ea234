// ppcx_ppc_exact.h -- the exact posterior-predictive tail probabilities and interval of a cell (ppcx_fit_ppc_exact): the
// Rao-Blackwellised form of the model's `generated quantities`. Given posterior draw i, the count of cell (g, s) is negative
// binomial with mean mu_i = e^{eta_i} and size phi_i; the posterior predictive distribution of the cell is therefore the equal-
// weight mixture of those n negative binomials, and its cdf the plain average of their cdfs (ppcx_nbcdf.h). No predictive count
// is drawn: what remains is the Monte-Carlo error of the posterior draws themselves. ppcx_fit_ppc answers the same question
// from one sampled count per draw and type-7 sample quantiles, which interpolate between integers; the quantiles here are the
// inverse-cdf quantiles of the distribution (integers), and the two agree in the limit of draws.
//
// Shared by the gfx950 kernel (ppcx_ppc_exact.hip) and the CPU check (tests/ppc_exact_host): the blocks below are
// `__host__ __device__`; ppc_exact_sweeps composes them once for both, and for ppcx_loo_exact.h; ppc_exact_cell_host at the end
// runs it sequentially.
//
// One cell from its count y and, per draw i = 0 .. n - 1, its linear predictor eta_i (loo_cell_eta) and sigma_raw_i:
//   0. ln phi_i = ln(truncation_compensation) - sigma_raw_i, phi_i = exp(ln phi_i): ppcx_fit_ppc's exp(-sigma_raw_i)
//      truncation_compensation up to rounding. A draw with invalid parameters (nb2_invalid, or e^{eta_i} not finite) makes every
//      statistic of the cell NaN, as a NaN ratio does in ppcx_loo.h; so does a continued fraction that reaches its cap.
//   1. mean = (sum_i mu_i) / n.
//   2. sd = sqrt((sum_i mu_i + mu_i^2 / phi_i) / n + (sum_i (mu_i - mean)^2) / n): the law of total variance, the variance of the
//      mu_i with ddof 0 in the two-pass form shifted by the mean of step 1.
//   3. p_le = (sum_i P_i(X <= y)) / n,  p_ge = (sum_i P_i(X >= y)) / n: nb2_log_tails per draw, each from its own sum.
//   4. F(k) = the mixture cdf at the integer k >= 0 from the two sums L = sum_i P_i(X <= k) and U = sum_i P_i(X > k) (each draw's
//      pair from nb2_cdf_pair: its smaller member directly from the continued fraction):  F = L / n where L <= U, else
//      1 - U / n. F(-1) = 0.
//      lower, upper = Q(p_lo), Q(p_hi), Q(p) the smallest integer k >= 0 with F(k) >= p, found by a DETERMINISTIC search:
//      c = floor(mean) and w = max(1, ceil(kPpcExactBracket sd)), both clipped to 2^30;
//      hi = c + w, and while F(hi) < p: w doubles, hi = c + w (at most to 2^31 - 2; F still below p there: NaN);
//      lo = c - w (the w the step before ended with), and while lo >= 0 and F(lo) >= p: hi = lo, w doubles, lo = c - w;
//      lo < 0 becomes -1;
//      then bisection on the integers: while hi - lo > 1, mid = lo + (hi - lo) / 2 goes to hi if F(mid) >= p, else to lo. Q = hi.
//      Every F is one sweep over the draws in a fixed order, so the result is a function of the cell's own draws only: the same
//      bits for any gene subset, gene batch or scratch batch.
//   5. y, excluded (reported only: the predictive does not depend on whether the cell is in the likelihood, an excluded cell
//      is treated exactly like any other), outside = (y < lower) | (y > upper) as 0 / 1 (NaN with the interval).
#pragma once
#include <stdint.h>
#include "ppcx_nbcdf.h"

namespace ppcx {

constexpr int kPpcExactFields = 9;             // mean, sd, p_le, p_ge, lower, upper, y, excluded, outside (include/ppcx.h)
constexpr double kPpcExactBracket = 4.0;       // the first bracket is mean +- this many sd
constexpr int kPpcExactMaxK = 2147483646;      // the largest count the search looks at

// step 0
PPCX_HD double ppc_exact_lnphi(double sigma_raw, double log_tc) { PPCX_NO_CONTRACT return log_tc - sigma_raw; }
PPCX_HD double ppc_exact_phi(double lnphi) { return exp(lnphi); }
PPCX_HD bool ppc_exact_invalid(double eta, double phi) { return nb2_invalid(eta, phi) || !isfinite(exp(eta)); }
// step 2, one draw's terms: *ev += mu + mu^2 / phi, *dv += (mu - mean)^2
PPCX_HD void ppc_exact_var_terms(double eta, double phi, double mean, double* ev, double* dv) {
  PPCX_NO_CONTRACT
  const double mu = exp(eta), d = mu - mean;
  *ev = mu + mu * mu / phi;
  *dv = d * d;
}
PPCX_HD double ppc_exact_sd(double ev_sum, double dv_sum, long n) { PPCX_NO_CONTRACT return sqrt(ev_sum / (double)n + dv_sum / (double)n); }
// step 4: F from the two sums
PPCX_HD double ppc_exact_F(double L, double U, long n) { PPCX_NO_CONTRACT return L <= U ? L / (double)n : 1.0 - U / (double)n; }
// the first bracket of the search
PPCX_HD void ppc_exact_bracket(double mean, double sd, int* c, int* w) {
  PPCX_NO_CONTRACT
  const double lim = 1073741824.0;
  const double cf = floor(mean), wf = ceil(kPpcExactBracket * sd);
  *c = cf < lim ? (int)cf : (int)lim;
  *w = wf < lim ? (wf > 1.0 ? (int)wf : 1) : (int)lim;
}
// The search of step 4 over any F (host: a sequential sweep; device: a workgroup sweep whose result every thread holds, so the
// control flow is uniform). Returns Q(p), or -1 where it is NaN (an F that is NaN, or still below p at kPpcExactMaxK). Every
// loop is bounded: w at most doubles to 2^31, the bisection halves an interval of at most 2^31.
template <class CDF>
PPCX_HD int ppc_exact_quantile(double p, int c, int w0, CDF F) {
  long w = w0;
  long hi = (long)c + w;
  for (int it = 0; it < 40; ++it) {
    const double f = F((int)hi);
    if (isnan(f)) return -1;
    if (f >= p) break;
    if (hi >= kPpcExactMaxK) return -1;
    w *= 2;
    hi = (long)c + w; if (hi > kPpcExactMaxK) hi = kPpcExactMaxK;
  }
  long lo = (long)c - w;
  for (int it = 0; it < 40 && lo >= 0; ++it) {
    const double f = F((int)lo);
    if (isnan(f)) return -1;
    if (!(f >= p)) break;
    hi = lo; w *= 2; lo = (long)c - w;
  }
  if (lo < 0) lo = -1;
  while (hi - lo > 1) {
    const long mid = lo + (hi - lo) / 2;
    const double f = F((int)mid);
    if (isnan(f)) return -1;
    if (f >= p) hi = mid; else lo = mid;
  }
  return (int)hi;
}
// step 5 and the layout of a cell's fields; lower / upper < 0: NaN
PPCX_HD void ppc_exact_store(double* o, double mean, double sd, double p_le, double p_ge, int lower, int upper, int y, bool excluded) {
  const bool ok = lower >= 0 && upper >= 0;
  o[0] = mean; o[1] = sd; o[2] = p_le; o[3] = p_ge;
  o[4] = ok ? (double)lower : NAN; o[5] = ok ? (double)upper : NAN;
  o[6] = (double)y; o[7] = excluded ? 1.0 : 0.0;
  o[8] = ok ? ((y < lower || y > upper) ? 1.0 : 0.0) : NAN;
}
PPCX_HD void ppc_exact_store_nan(double* o, int y, bool excluded) {
  for (int f = 0; f < kPpcExactFields; ++f) o[f] = NAN;
  o[6] = (double)y; o[7] = excluded ? 1.0 : 0.0;
}


// a weighted term of a sum (w = 1 in the uniform cell of ppcx_loo_exact.h: the product is exact)
PPCX_HD double loo_exact_term(double w, double f) { PPCX_NO_CONTRACT return w * f; }

// Steps 1 - 5 of this header and steps 2 - 6 of ppcx_loo_exact.h, once, over any "sum over the draws": sums(f, s) leaves in
// s[0 .. K) the sums over the draws i of w_i t_k, where f(eta_i, ln phi_i, t) fills the draw's K terms and returns the
// continued-fraction steps it took (0 where there are none). The operation carries the weight -- none here, loo_exact_term(w_i, .)
// in ppcx_loo_exact.h -- the order (host: sequential; device: a workgroup's strided sweep and block_sum, so that every thread
// holds the same sums and the control flow is uniform) and what becomes of the step counts. den: what every sum is divided by
// (n, or 1 under normalised weights). Where `store`, the nine fields go to o (NaN where a sum or an interval end is NaN);
// returns whether they are numbers.
template <class Sums>
PPCX_HD bool ppc_exact_sweeps(const Sums& sums, int y, bool excluded, long den, double p_lo, double p_hi, bool store, double* o) {
  PPCX_NO_CONTRACT
  double sm[1], var[2], tails[2];
  sums([](double eta, double, double* t) { t[0] = exp(eta); return 0; }, sm);
  const double mean = sm[0] / (double)den;
  sums([mean](double eta, double lp, double* t) { ppc_exact_var_terms(eta, ppc_exact_phi(lp), mean, &t[0], &t[1]); return 0; }, var);
  const double sd = ppc_exact_sd(var[0], var[1], den);
  sums([y](double eta, double lp, double* t) { return nb2_log_tails_ln(y, eta, ppc_exact_phi(lp), lp, &t[0], &t[1]); }, tails);
  // the interval: every F is one sweep
  auto F = [&](int k) {
    double LU[2];
    sums([k](double eta, double lp, double* t) {
      double pm; int it;
      nb2_cdf_pair(k, eta, ppc_exact_phi(lp), lp, &t[0], &t[1], &pm, &it);
      return it;
    }, LU);
    return ppc_exact_F(LU[0], LU[1], den);
  };
  int c, w;
  ppc_exact_bracket(mean, sd, &c, &w);
  const int lower = ppc_exact_quantile(p_lo, c, w, F), upper = ppc_exact_quantile(p_hi, c, w, F);
  const bool ok = !(isnan(tails[0]) || isnan(tails[1]) || lower < 0 || upper < 0);
  if (store) {
    if (ok) ppc_exact_store(o, mean, sd, tails[0] / (double)den, tails[1] / (double)den, lower, upper, y, excluded);
    else ppc_exact_store_nan(o, y, excluded);
  }
  return ok;
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
namespace ppcx {
// the sums of ppc_exact_sweeps for the CPU checks: sequential, under the weights w (null: none), ln phi formed on the way;
// *max_iters: the largest number of continued-fraction steps any evaluation took
struct ExactHostSums {
  const double* w; const double* eta; const double* sigma_raw; double log_tc; long n; int* max_iters;
  template <class F, int K>
  void operator()(F f, double (&s)[K]) const {
    PPCX_NO_CONTRACT
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (long i = 0; i < n; ++i) {
      double t[K];
      const int it = f(eta[i], ppc_exact_lnphi(sigma_raw[i], log_tc), t);
      if (it > *max_iters) *max_iters = it;
      for (int k = 0; k < K; ++k) s[k] += w ? loo_exact_term(w[i], t[k]) : t[k];
    }
  }
};
// the whole spec for one cell, sequentially, for the CPU check: out[kPpcExactFields]. max_iters (may be null): the largest
// number of continued-fraction steps any evaluation took.
inline void ppc_exact_cell_host(const double* eta, const double* sigma_raw, long n, int y, bool excluded, double tc, double p_lo,
                                double p_hi, double* out, int* max_iters = nullptr) {
  const double log_tc = log(tc);
  int mx = 0;
  for (long i = 0; i < n; ++i)
    if (ppc_exact_invalid(eta[i], ppc_exact_phi(ppc_exact_lnphi(sigma_raw[i], log_tc)))) { ppc_exact_store_nan(out, y, excluded); return; }
  ppc_exact_sweeps(ExactHostSums{nullptr, eta, sigma_raw, log_tc, n, &mx}, y, excluded, n, p_lo, p_hi, true, out);
  if (max_iters) *max_iters = mx;
}
}  // namespace ppcx
#endif
