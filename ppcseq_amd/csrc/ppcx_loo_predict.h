// ppcx_loo_predict.h -- the leave-one-out predictive interval and LOO-PIT per observed cell of a NUTS fit (ppcx_fit_loo_predict):
// for cell (g, s), the distribution of its count under the posterior that has not seen the cell -- what
// loo::E_loo(yrep, psis_object, type = "quantile" / "mean") and bayesplot's ppc_loo_intervals / ppc_loo_pit give an rstan user,
// and what ppcseq's second fit approximates. The weights are those of ppcx_loo.h (PSIS on r = -ll); here every draw carries its
// own weight, because every draw carries its own predictive count.
//
// Shared by the gfx950 kernel (ppcx_loo_predict.hip) and the CPU check (tests/loo_predict_host): the blocks below are
// `__host__ __device__`; loo_predict_cell_host at the end is their sequential composition.
//
// One cell from its log-likelihoods ll[0 .. n), its predictive counts x[0 .. n) (draw i: neg_binomial_2_log_rng(eta_i,
// truncation_compensation exp(-sigma_raw_i)) on the Philox address (seed, g S + s, i): the integers of ppcx_fit_ppc's counts_rng
// with n_gen = 0, resample = 0) and its observed count y:
//   1. ratios r = -ll, N, the tail length M, k-hat, sigma and the cutoff as ppcx_loo.h steps 1 - 2. A NaN ratio, +Inf, or an
//      invalid predictive draw (2^31 - 1): every field NaN. A ratio of -Inf takes no part: weight 0, and its count is not a
//      drawn value.
//   2. The log weight of draw i. The participating draws are ordered by ratio with a STABLE sort (ties keep draw order); the tail
//      is the last M of that order. Where the tail is smoothed (loo_smooth_ok), the draw at tail position j = 1 .. M gets
//      loo_smoothed(j, M, ..), every other draw r_i - mx; all truncated at 0. Hence the TIE RULE: among draws tied at the cutoff
//      those with the highest draw indices are in the tail, and tied tail draws take their positions in draw order. A draw's
//      position comes from the sorted keys K[0 .. M] of the M + 1 largest ratios (K[0] the cutoff, `want` copies of its key
//      among them) by binary search, plus, for a key that occurs more than once, the number of earlier draws with that key
//      (loo_predict_tail_pos).
//   3. w_i = exp(lw_i - max lw) / sum; F(v) = sum_i w_i 1[x_i <= v].
//      mean = sum w_i x_i;  pit_lt = sum w_i 1[x_i < y];  pit_le = F(y)   (the two ends of the randomised LOO-PIT);
//      lower, upper = Q(p_lo), Q(p_hi): v* the smallest drawn value with F(v*) >= p (the largest drawn value if rounding keeps F
//      below p). If no drawn value is below v*, Q = v*; else with v- the largest drawn value below v*,
//      Q = v- + (v* - v-) (p - F(v-)) / (F(v*) - F(v-))   (loo's weighted quantile on the distinct values);
//      khat as ppcx_fit_loo.
//   4. A cell the model excludes is already held out: uniform weights, khat = NaN, mean = (sum x_i) / n (an integer sum),
//      lower / upper the type-7 quantiles of x as ppcx_fit_ppc's kernels take them (type7, ppcx_ppc.h), pit_lt = #{x_i < y} / n,
//      pit_le = #{x_i <= y} / n. With phi formed by the same ppc_phi these are ppcx_fit_ppc's mean,
//      .lower and .upper bit for bit (the log-likelihood decides nothing but NaN).
// Every reduction runs in a fixed order: a cell's fields depend on its own column only.
#pragma once
#include <stdint.h>
#include "ppcx_loo.h"
#include "ppcx_ppc.h"

namespace ppcx {

constexpr int kLooPredictFields = 6;           // mean, lower, upper, pit_lt, pit_le, khat (include/ppcx.h PPCX_LOO_PREDICT_FIELDS)

// first index j in the ascending K[0 .. M] with K[j] >= k (k is one of them)
PPCX_HD int loo_predict_lower_bound(const uint64_t* K, int M, uint64_t k) {
  int lo = 0, hi = M;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (K[mid] < k) lo = mid + 1; else hi = mid; }
  return lo;
}
// whether the key k (> the cutoff's) occurs more than once among the M + 1 largest: then `before` of loo_predict_tail_pos counts
PPCX_HD bool loo_predict_tied(const uint64_t* K, int M, int lb) { return lb < M && K[lb + 1] == K[lb]; }
// Tail position 1 .. M of a draw with ratio key k, or 0 outside the tail (step 2). cut_key: the cutoff's key, `want` copies of
// it among K[0 .. M], n_eq among all draws; before: the earlier draws (smaller index) with the same key (needed where the key
// is the cutoff's and want > 1, or loo_predict_tied).
PPCX_HD int loo_predict_tail_pos(uint64_t k, const uint64_t* K, int M, uint64_t cut_key, int want, long n_eq, long before) {
  if (k < cut_key) return 0;
  if (k == cut_key) {                            // the last want - 1 copies in draw order are in the tail, at 1 .. want - 1
    const long first_in = n_eq - (long)(want - 1);
    return before >= first_in ? (int)(before - first_in) + 1 : 0;
  }
  return loo_predict_lower_bound(K, M, k) + (int)before;
}
// the log weight of a draw: raw, or smoothed at tail position j > 0; truncated at 0; -Inf for a draw that takes no part
PPCX_HD double loo_predict_lw(double r, double mx, int j, int M, double khat, double sigma, double ec) {
  PPCX_NO_CONTRACT
  if (r == -INFINITY) return -INFINITY;
  const double lw = j > 0 ? loo_smoothed(j, M, khat, sigma, ec) : r - mx;
  return lw > 0.0 ? 0.0 : lw;
}
// Q(p) between the support points v- < v* with F(v-) = Fm, F(v*) = Fs
PPCX_HD double loo_predict_interp(double vm, double vs, double Fm, double Fs, double p) {
  PPCX_NO_CONTRACT
  return vm + (vs - vm) * (p - Fm) / (Fs - Fm);
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
namespace ppcx {
// the whole spec for one cell, sequentially, for the CPU check: out[kLooPredictFields]
inline void loo_predict_cell_host(const double* ll, const int32_t* x, long n, int y, double r_eff, bool excluded, double p_lo,
                                  double p_hi, double* out) {
  auto all_nan = [&]() { for (int f = 0; f < kLooPredictFields; ++f) out[f] = NAN; };
  const double pr[2] = {p_lo, p_hi};
  for (long i = 0; i < n; ++i) {
    const double r = -ll[i];
    if (isnan(r) || (!excluded && r == INFINITY) || x[i] == kPpcInvalid) { all_nan(); return; }
  }
  if (excluded) {
    double sum = 0.0; long lt = 0, le = 0;
    for (long i = 0; i < n; ++i) { sum += (double)x[i]; lt += x[i] < y; le += x[i] <= y; }
    std::vector<int32_t> xs(x, x + n);
    std::sort(xs.begin(), xs.end());
    out[0] = sum / (double)n;
    for (int k = 0; k < 2; ++k) {
      double h; long lo;
      type7_rank(n, pr[k], &h, &lo);
      out[1 + k] = type7(h, lo, n, (double)xs[lo], (double)xs[lo + 1 < n ? lo + 1 : lo]);
    }
    out[3] = (double)lt / (double)n; out[4] = (double)le / (double)n; out[5] = NAN;
    return;
  }
  // ---- the sorted ratios of the participating draws, the tail, the keys of the M + 1 largest
  std::vector<double> rs;
  for (long i = 0; i < n; ++i) if (ll[i] != INFINITY) rs.push_back(-ll[i]);
  const long N = (long)rs.size();
  if (N == 0) { all_nan(); return; }
  std::sort(rs.begin(), rs.end());
  const double mx = rs[N - 1];
  const int M = psis_tail_len(N, r_eff);
  double khat = INFINITY, sigma = 0.0, ec = 0.0;
  bool smooth = false;
  std::vector<uint64_t> K;
  int want = 0; long n_eq = 0;
  if (M >= 5 && M < N && rs[N - M] != mx) {
    const PsisTailHost t = psis_tail_host(rs.data(), N, M);
    sigma = -t.k_mean / t.theta_hat; ec = t.ec;
    khat = psis_adjust(t.k_mean, M);
    smooth = loo_smooth_ok(khat, sigma);
    for (int j = 0; j <= M; ++j) K.push_back(psis_key(rs[N - M - 1 + j]));
    for (int j = 0; j <= M; ++j) want += K[j] == K[0];
    for (long i = 0; i < N; ++i) n_eq += psis_key(rs[i]) == K[0];
  }
  // ---- the weight of every draw (step 2), by the kernel's rule
  std::vector<double> w(n);
  double mxw = -INFINITY;
  for (long i = 0; i < n; ++i) {
    const double r = -ll[i];
    int j = 0;
    if (smooth && r != -INFINITY) {
      const uint64_t k = psis_key(r);
      long before = 0;
      if (k >= K[0]) for (long i2 = 0; i2 < i; ++i2) before += psis_key(-ll[i2]) == k;
      j = loo_predict_tail_pos(k, K.data(), M, K[0], want, n_eq, before);
    }
    w[i] = loo_predict_lw(r, mx, j, M, khat, sigma, ec);
    mxw = w[i] > mxw ? w[i] : mxw;
  }
  double sw = 0.0;
  for (long i = 0; i < n; ++i) { w[i] = exp(w[i] - mxw); sw += w[i]; }
  for (long i = 0; i < n; ++i) w[i] /= sw;
  // ---- step 3
  double mean = 0.0, plt = 0.0, ple = 0.0;
  for (long i = 0; i < n; ++i) { mean += w[i] * (double)x[i]; if (x[i] < y) plt += w[i]; if (x[i] <= y) ple += w[i]; }
  std::vector<int32_t> vals;
  for (long i = 0; i < n; ++i) if (ll[i] != INFINITY) vals.push_back(x[i]);
  std::sort(vals.begin(), vals.end());
  vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
  auto F = [&](int32_t v) { double s = 0.0; for (long i = 0; i < n; ++i) if (x[i] <= v) s += w[i]; return s; };
  out[0] = mean; out[3] = plt; out[4] = ple; out[5] = khat;
  for (int k = 0; k < 2; ++k) {
    size_t q = 0;
    while (q + 1 < vals.size() && !(F(vals[q]) >= pr[k])) ++q;
    out[1 + k] = q == 0 ? (double)vals[0]
                        : loo_predict_interp((double)vals[q - 1], (double)vals[q], F(vals[q - 1]), F(vals[q]), pr[k]);
  }
}
}  // namespace ppcx
#endif
