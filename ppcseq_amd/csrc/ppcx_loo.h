// ppcx_loo.h -- PSIS-LOO per observed cell of a NUTS fit (ppcx_fit_loo, ppcx_fit_get_log_lik): what rstan::loo(fit) and
// loo::loo(log_lik, r_eff) report per observation. Vehtari, Gelman, Gabry (2017), "Practical Bayesian model evaluation using
// leave-one-out cross-validation and WAIC"; the tail fit is ppcx_psis.h's (Vehtari, Simpson, Gelman, Yao, Gabry 2024).
//
// Shared by the gfx950 kernels (ppcx_loo.hip) and the CPU check (tests/loo_host): the blocks below are `__host__ __device__`;
// loo_cell_host at the end is their sequential composition, the kernel composes them with workgroup-parallel loops.
//
// Log-likelihood of a non-excluded or excluded cell (g, s) at draw theta:
//   ll = neg_binomial_2_log_lpmf(y | eta, phi) with every constant kept, eta = exposure_s + X_s . alpha_g,
//   phi = exp(-sigma_raw_g): what a Stan `generated quantities { log_lik }` block holds. With t = eta + sigma_raw, w = 1 + e^t
//   (ppcx_disp.h):  ll = y eta - y - (y + phi) ln w + Fh - lgamma(y + 1),  Fh = lgamma(y + phi) - lgamma(phi) + y sigma_raw + y
//   the cell's own Fh (disp_point / disp_cell), never the per-gene tables (they hold sums over a gene).
//
// PSIS-LOO of one cell from its column ll[0 .. n) (loo's psis() on the log ratios r = -ll, then loo's pointwise columns):
//   a NaN ratio, or +Inf (ll = -Inf): every field NaN. A ratio of -Inf (ll = +Inf) takes no part; N = the other draws.
//   1. M = ceil(min(0.2 N, 3 sqrt(N / r_eff))) (r_eff = 1 unless the caller gives one).
//   2. In the frame shifted by the largest ratio mx: the tail is the M largest ratios, the cutoff c the (M + 1)-th largest.
//      M < 5, or the M tail values all equal: k-hat = +Inf and the raw weights. Otherwise ppcx_psis.h steps 2 - 4 give k-hat
//      and theta^; sigma = -k / theta^ with the mean k BEFORE the adjustment. Where k-hat is finite and sigma > 0, the j-th
//      smallest tail ratio (j = 1 .. M) is replaced by log(qgpd((j - 1/2) / M; k-hat, sigma) + exp(c - mx)),
//      qgpd(p) = sigma expm1(-k-hat log1p(-p)) / k-hat; otherwise the raw tail stays.
//   3. every log weight lw is truncated at 0 (the largest raw one); the weights are normalised by logsumexp(lw).
//   4. elpd_loo = logsumexp(lw + ll) - logsumexp(lw); lpd = logsumexp(ll) - log N; p_loo = lpd - elpd_loo;
//      looic = -2 elpd_loo; khat = k-hat.
//   Tied ratios have equal ll, so which of them receives which smoothed weight does not change any sum here. It does where a
//   draw carries more than its ll: ppcx_loo_predict.h step 2 fixes the order (a stable sort: tied draws in draw order).
// An excluded cell (not in the likelihood at the time of the call) is already held out: elpd_loo = lpd, p_loo = 0,
// looic = -2 lpd, khat = NaN (a NaN ll: all NaN; ll = +Inf takes no part).
//
// The Monte-Carlo standard error of elpd_loo and the effective sample size of the PSIS weights (ppcx_fit_loo_mcse: as loo::loo
// reports mcse_elpd_loo -- deterministic Blom-score form, n_samples = 1000 -- and psis_n_eff; restated from the published
// package, not run against it). For a cell that is not NaN, with w_i its normalised weights (those behind elpd_loo: step 3,
// raw where khat = +Inf; uniform 1 / N for an excluded cell), sum w_i = 1, and r its r_eff (1 without):
//   5. n_eff = r / sum w_i^2 (an excluded cell: N r, formed as that product).
//   6. c = sqrt(sum w_i^2 expm1(ll_i - e)^2), e = elpd_loo: loo's sd_epd / E_epd, in the shifted frame, which stays defined
//      where exp(ll) underflows. e is elpd_loo brought into [min ll, max ll], where it lies but for the rounding of the two
//      logsumexps: a constant column then gives c = 0 exactly.
//   7. z_j = 1 + c blom_z(j, 1000), j = 1 .. 1000 (ppcx_summary.h: Phi^-1((j - 3/8) / (1000 + 1/4)); loo's E + sd z over E);
//      v = the variance (ddof 1) of log1p(c blom_z(j, 1000)) over the j with z_j > 0 (at least 500 of them).
//   8. mcse_elpd_loo = sqrt(v / r).
//   A cell that is NaN above, or without a participating draw, is NaN in both.
// Every reduction runs in a fixed order: a cell's fields depend on its own column only.
#pragma once
#include <stdint.h>
#include "ppcx_math.h"
#include "ppcx_disp.h"
#include "ppcx_psis.h"
#include "ppcx_summary.h"

namespace ppcx {

constexpr int kLooFields = 4;                  // elpd_loo, p_loo, looic, khat (include/ppcx.h PPCX_LOO_FIELDS)
constexpr int kLooMcseFields = 6;              // those, mcse_elpd_loo, n_eff (include/ppcx.h PPCX_LOO_MCSE_FIELDS)
constexpr int kLooMcseScores = 1000;           // loo's n_samples: the Blom scores of step 7

// ln(1 + e^t) for every t
PPCX_HD double loo_log1pexp(double t) {
  PPCX_NO_CONTRACT
  return t > 0.0 ? t + log1p(exp(-t)) : log1p(exp(t));
}
// the cell's log-likelihood at one draw (y >= 0)
PPCX_HD double loo_ll(int y, double eta, double sigma_raw) {
  PPCX_NO_CONTRACT
  const DispPoint p = disp_point(sigma_raw);
  double F, Dh;
  disp_cell(y, p, &F, &Dh);
  const double yd = (double)y;
  const double lw = loo_log1pexp(eta + sigma_raw);
  return yd * eta - yd - (yd + p.phi) * lw + F - lgamma_int1(yd);
}
// the smoothed log weight of tail position j = 1 .. M (shifted frame), given k-hat, sigma and exp(cutoff - mx)
PPCX_HD double loo_smoothed(int j, int M, double khat, double sigma, double ec) {
  PPCX_NO_CONTRACT
  const double p = ((double)j - 0.5) / (double)M;
  const double q = sigma * expm1(-khat * log1p(-p)) / khat;
  return log(q + ec);
}
// whether the tail is replaced (step 2)
PPCX_HD bool loo_smooth_ok(double khat, double sigma) { return isfinite(khat) && sigma > 0.0; }

// ---- steps 5 - 8
// e of step 6: elpd_loo within the range of the participating ll
PPCX_HD double loo_mcse_frame(double elpd, double ll_min, double ll_max) { return fmin(fmax(elpd, ll_min), ll_max); }
// one draw's terms (mult copies): w = exp(lw - lse) its normalised weight; *w2 += w^2, *c2 += (w expm1(ll - e))^2
PPCX_HD void loo_mcse_add(double lw, double ll, double lse, double e, double mult, double* w2, double* c2) {
  PPCX_NO_CONTRACT
  const double w = exp(lw - lse);
  const double d = w * expm1(ll - e);
  *w2 += mult * (w * w);
  *c2 += mult * (d * d);
}
// one draw's term of an excluded cell before the division by N^2: expm1(ll - e)^2
PPCX_HD double loo_mcse_uniform_term(double ll, double e) {
  PPCX_NO_CONTRACT
  const double d = expm1(ll - e);
  return d * d;
}
PPCX_HD double loo_mcse_uniform_c2(double sum, long N) { return sum / ((double)N * (double)N); }
// step 7, score j = 1 .. kLooMcseScores: log1p(c blom_z(j)), NaN where z_j <= 0 (the score takes no part)
PPCX_HD double loo_mcse_score(int j, double c) {
  PPCX_NO_CONTRACT
  const double t = c * blom_z((double)j, kLooMcseScores);
  return 1.0 + t > 0.0 ? log1p(t) : NAN;
}
// step 8 from the sum of squared deviations of the cnt scores that take part
PPCX_HD double loo_mcse_from(double ss, double cnt, double r_eff) { return cnt >= 2.0 ? sqrt(ss / (cnt - 1.0) / r_eff) : NAN; }

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
namespace ppcx {
inline double loo_logsumexp_host(const std::vector<double>& v) {
  double mx = -INFINITY;
  for (double x : v) mx = x > mx ? x : mx;
  if (mx == -INFINITY) return -INFINITY;
  double s = 0.0;
  for (double x : v) s += exp(x - mx);
  return mx + log(s);
}
// steps 7 - 8, sequentially
inline double loo_mcse_blom_host(double c, double r_eff) {
  std::vector<double> x;
  for (int j = 1; j <= kLooMcseScores; ++j) { const double v = loo_mcse_score(j, c); if (!isnan(v)) x.push_back(v); }
  double s = 0.0, ss = 0.0;
  for (double v : x) s += v;
  const double mean = s / (double)x.size();
  for (double v : x) ss += (v - mean) * (v - mean);
  return loo_mcse_from(ss, (double)x.size(), r_eff);
}
// the whole spec for one cell, sequentially, for the CPU check: out[kLooFields], or out[kLooMcseFields] with mcse
inline void loo_cell_host(const double* ll, long n, double r_eff, bool excluded, double* out, bool mcse = false) {
  std::vector<double> l;
  l.reserve((size_t)n);
  if (mcse) out[4] = out[5] = NAN;
  for (long i = 0; i < n; ++i) {
    const double r = -ll[i];
    if (isnan(r) || (!excluded && r == INFINITY)) { out[0] = out[1] = out[2] = out[3] = NAN; return; }
    if (r != -INFINITY) l.push_back(ll[i]);
  }
  const long N = (long)l.size();
  const double lpd = N > 0 ? loo_logsumexp_host(l) - log((double)N) : NAN;
  double ll_min = INFINITY, ll_max = -INFINITY;
  for (double x : l) { ll_min = x < ll_min ? x : ll_min; ll_max = x > ll_max ? x : ll_max; }
  if (excluded) {
    out[0] = lpd; out[1] = 0.0; out[2] = -2.0 * lpd; out[3] = NAN;
    if (mcse && N > 0) {
      const double e = loo_mcse_frame(lpd, ll_min, ll_max);
      double sum = 0.0;
      for (double x : l) sum += loo_mcse_uniform_term(x, e);
      out[4] = loo_mcse_blom_host(sqrt(loo_mcse_uniform_c2(sum, N)), r_eff);
      out[5] = (double)N * r_eff;
    }
    return;
  }
  // ratios sorted ascending, each with its draw's ll (tied ratios have equal ll)
  std::vector<double> r(N);
  for (long i = 0; i < N; ++i) r[i] = -l[i];
  std::sort(r.begin(), r.end());
  const double mx = r[N - 1];
  std::vector<double> lw(N);
  for (long i = 0; i < N; ++i) lw[i] = r[i] - mx;
  const int M = psis_tail_len(N, r_eff);
  double khat = INFINITY;
  if (M >= 5 && M < N && r[N - M] != mx) {
    const PsisTailHost t = psis_tail_host(r.data(), N, M);
    const double sigma = -t.k_mean / t.theta_hat;
    khat = psis_adjust(t.k_mean, M);
    if (loo_smooth_ok(khat, sigma))
      for (int j = 1; j <= M; ++j) lw[N - M + j - 1] = loo_smoothed(j, M, khat, sigma, t.ec);
  }
  std::vector<double> a(N);
  for (long i = 0; i < N; ++i) { lw[i] = lw[i] > 0.0 ? 0.0 : lw[i]; a[i] = lw[i] - r[i]; }
  const double lse = loo_logsumexp_host(lw);
  const double elpd = loo_logsumexp_host(a) - lse;
  out[0] = elpd; out[1] = lpd - elpd; out[2] = -2.0 * elpd; out[3] = khat;
  if (mcse) {
    const double e = loo_mcse_frame(elpd, ll_min, ll_max);
    double w2 = 0.0, c2 = 0.0;
    for (long i = 0; i < N; ++i) loo_mcse_add(lw[i], -r[i], lse, e, 1.0, &w2, &c2);
    out[4] = loo_mcse_blom_host(sqrt(c2), r_eff);
    out[5] = r_eff / w2;
  }
}
}  // namespace ppcx
#endif
