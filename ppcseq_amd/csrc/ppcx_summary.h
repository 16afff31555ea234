// ppcx_summary.h -- the per-column statistics of a fit summary (ppcx_fit_summary): the plain summary, the rank-normalised
// split R-hat and the bulk / tail effective sample sizes of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021),
// "Rank-normalization, folding, and localization", with the Geyer truncation as rstan's monitor() writes it.
//
// Shared by the gfx950 kernel (ppcx_summary.hip, one workgroup per column) and the CPU check (tests/summary_host): the
// building blocks below are `__host__ __device__`; summary_column_host at the end is the sequential composition of them
// that the CPU check runs, and the kernel composes the same blocks with workgroup-parallel loops.
//
// Spec of one column x of a fit with M chains of n kept draws (chain-major, x[c * n + i]):
//   mean, sd (ddof 1), q05 / q50 / q95 (type 7) over all M n draws;
//   split chains: n' = floor(n / 2), chain c gives sequences 2c (its first n' draws) and 2c + 1 (its last n'; an odd n drops
//   the middle draw), m = 2M sequences, N = m n' values;
//   z = Phi^-1((r - 3/8) / (N + 1/4)) of the average ranks r over the N split values (Blom);
//   rhat = max(R-hat(z), R-hat(z of |x - median|)) (fmax: a side without variance gives way); ess_bulk = ESS(z); ess_tail = min(ESS(1[x <= q05]), ESS(1[x <= q95]))
//   with median, q05, q95 type 7 over the split values;
//   a non-finite draw: every field NaN; split values all equal or n' < 2: rhat, ess_bulk, ess_tail NaN; an indicator
//   sequence without variance: its ESS NaN (ess_tail takes the other side, NaN only when both are).
#pragma once
#include "ppcx_math.h"

#if defined(__clang__)
#define PPCX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PPCX_NO_CONTRACT
#endif

namespace ppcx {

enum SummaryField : int { SUM_MEAN = 0, SUM_SD, SUM_Q05, SUM_Q50, SUM_Q95, SUM_RHAT, SUM_ESS_BULK, SUM_ESS_TAIL, SUM_FIELDS };

// split value k (0 <= k < 2 M n') -> index of the draw in the chain-major column [M][n]
PPCX_HD long split_source(long k, int nh, int n) {
  const long j = k / nh, i = k - j * nh;
  return (j >> 1) * (long)n + ((j & 1) ? (long)(n - nh) : 0L) + i;
}

// type-7 quantile of the sorted s[0 .. N) (R's default; inference.quantile7): s[lo] + (h - lo) (s[lo + 1] - s[lo]),
// h = (N - 1) p, evaluated without contraction so that every build gives the same bits
PPCX_HD double quantile7_sorted(const double* s, long N, double p) {
  PPCX_NO_CONTRACT
  const double h = (double)(N - 1) * p;
  const double fl = floor(h);
  const long lo = (long)fl;
  if (lo >= N - 1) return s[N - 1];
  const double a = s[lo], b = s[lo + 1];
  const double w = h - fl;
  const double d = b - a;
  const double t = w * d;
  return a + t;
}

// average rank (1-based, ties share their mean rank) of v among the sorted s[0 .. N): (#{< v} + #{<= v} + 1) / 2
PPCX_HD double average_rank(const double* s, long N, double v) {
  long lo = 0, hi = N;                          // first index with s >= v
  while (lo < hi) { const long mid = (lo + hi) >> 1; if (s[mid] < v) lo = mid + 1; else hi = mid; }
  const long below = lo;
  long upto = lo;                               // first index with s > v: usually below + 1 (no tie)
  if (upto < N && !(s[upto] > v)) {
    if (upto + 1 >= N || s[upto + 1] > v) upto = upto + 1;
    else {
      long a = upto + 1, b = N;
      while (a < b) { const long mid = (a + b) >> 1; if (s[mid] > v) b = mid; else a = mid + 1; }
      upto = a;
    }
  }
  return 0.5 * (double)(below + upto + 1);
}

// Phi^-1(p), 0 < p < 1: Acklam's rational approximation (relative error < 1.2e-9) and one Halley step on erfc, taken in the
// lower tail (p > 1/2 through 1 - p, exact there) so that erfc is evaluated where it is accurate: ~1e-16 relative
PPCX_HD double ndtri_lower(double q) {                 // 0 < q <= 1/2
  const double a1 = -3.969683028665376e+01, a2 = 2.209460984245205e+02, a3 = -2.759285104469687e+02,
               a4 = 1.383577518672690e+02, a5 = -3.066479806614716e+01, a6 = 2.506628277459239e+00;
  const double b1 = -5.447609879822406e+01, b2 = 1.615858368580409e+02, b3 = -1.556989798598866e+02,
               b4 = 6.680131188771972e+01, b5 = -1.328068155288572e+01;
  const double c1 = -7.784894002430293e-03, c2 = -3.223964580411365e-01, c3 = -2.400758277161838e+00,
               c4 = -2.549732539343734e+00, c5 = 4.374664141464968e+00, c6 = 2.938163982698783e+00;
  const double d1 = 7.784695709041462e-03, d2 = 3.224671290700398e-01, d3 = 2.445134137142996e+00, d4 = 3.754408661907416e+00;
  double x;
  if (q < 0.02425) {
    const double r = sqrt(-2.0 * log(q));
    x = (((((c1 * r + c2) * r + c3) * r + c4) * r + c5) * r + c6) / ((((d1 * r + d2) * r + d3) * r + d4) * r + 1.0);
  } else {
    const double u = q - 0.5, r = u * u;
    x = (((((a1 * r + a2) * r + a3) * r + a4) * r + a5) * r + a6) * u /
        (((((b1 * r + b2) * r + b3) * r + b4) * r + b5) * r + 1.0);
  }
  const double e = 0.5 * erfc(-x * 0.70710678118654752440) - q;
  const double u = e * 2.50662827463100050242 * exp(0.5 * x * x);
  return x - u / (1.0 + 0.5 * x * u);
}
PPCX_HD double ndtri(double p) { return p > 0.5 ? -ndtri_lower(1.0 - p) : ndtri_lower(p); }
PPCX_HD double blom_z(double rank, long N) { return ndtri((rank - 0.375) / ((double)N + 0.25)); }

// R-hat of m sequences of n' values from the variance of their means (ddof 1) and the mean of their variances (ddof 1):
// B = n' var_means, W = mean_var, sqrt((B / W + n' - 1) / n')
PPCX_HD double rhat_from(double var_means, double mean_var, int nh) {
  return sqrt(((double)nh * var_means / mean_var + (double)nh - 1.0) / (double)nh);
}
// the pooled variance of the ESS estimator: mean_var (n' - 1) / n' + var_means
PPCX_HD double var_plus_of(double var_means, double mean_var, int nh) { return mean_var * ((double)nh - 1.0) / (double)nh + var_means; }
// rho[t] from the chain-averaged autocovariance at lag t (mean over sequences of (1 / n') sum_i c_i c_{i+t})
PPCX_HD double rho_of(double acov_mean, double mean_var, double var_plus) { return 1.0 - (mean_var - acov_mean) / var_plus; }

// Geyer's initial positive + monotone sequence (rstan monitor(): ess_rfun), fed pair by pair so that the caller computes the
// autocorrelations only as far as the truncation needs them:
//   rho^[0] = 1, rho^[1] = rho[1]; t = 0; while t < n' - 5 and even + odd > 0: t += 2, even = rho[t], odd = rho[t + 1], the
//   pair kept in rho^ when even + odd >= 0; max_t = t; rho^[max_t] = even when even > 0; monotone: for t = 2, 4, .. <= max_t - 2
//   a pair whose sum exceeds the previous pair's takes the previous pair's mean (so pair sums are a running minimum);
//   tau = -1 + 2 sum_{k < max_t} rho^[k] + rho^[max_t], at least 1 / log10(N); ESS = N / tau.
// Use: g.start(nh, rho1); while (g.wants()) g.feed(rho[g.next()], rho[g.next() + 1]); ess = g.ess(N)
struct Geyer {
  int nh, t;
  double even, odd;
  double pair;        // rho^[t] + rho^[t + 1] of the current pair (0 when it was not kept)
  bool kept;
  double acc;         // sum of the monotone pair sums before the current pair
  double prev;        // the last of them
  PPCX_HD void start(int nh_, double rho1) { nh = nh_; t = 0; even = 1.0; odd = rho1; pair = 1.0 + rho1; kept = true; acc = 0.0; prev = 0.0; }
  PPCX_HD bool wants() const { return t < nh - 5 && even + odd > 0.0; }
  PPCX_HD int next() const { return t + 2; }
  PPCX_HD void feed(double e, double o) {
    const double p = t == 0 ? pair : (pair < prev ? pair : prev);   // the current pair is now below max_t: it enters the sum
    acc += p; prev = p;
    t += 2; even = e; odd = o;
    kept = e + o >= 0.0;
    pair = kept ? e + o : 0.0;
  }
  PPCX_HD double tau(long N) const {
    const double last = (kept || even > 0.0) ? even : 0.0;           // rho^[max_t]
    const double tau_ = -1.0 + 2.0 * acc + last;
    const double floor_ = 1.0 / log10((double)N);
    return tau_ > floor_ ? tau_ : floor_;
  }
  PPCX_HD double ess(long N) const { return (double)N / tau(N); }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the sequential composition (CPU check): x chain-major [M][n], out[SUM_FIELDS]; work: 3 M n doubles
inline void summary_sort(double* s, long n) {           // heap sort: no library dependence, any order of equal values
  auto sift = [&](long i, long len) {
    for (;;) { long c = 2 * i + 1; if (c >= len) return; if (c + 1 < len && s[c + 1] > s[c]) ++c; if (!(s[c] > s[i])) return;
               const double t = s[i]; s[i] = s[c]; s[c] = t; i = c; }
  };
  for (long i = n / 2 - 1; i >= 0; --i) sift(i, n);
  for (long e = n - 1; e > 0; --e) { const double t = s[0]; s[0] = s[e]; s[e] = t; sift(0, e); }
}
// R-hat (and, when ess != null, the ESS) of m sequences of nh values z[j * nh + i]; z is centred in place
inline double summary_seq_host(double* z, int m, int nh, double* ess) {
  double mm = 0.0, mv = 0.0;
  double* means = new double[m];
  for (int j = 0; j < m; ++j) {
    double s = 0.0; for (int i = 0; i < nh; ++i) s += z[(long)j * nh + i];
    means[j] = s / nh;
    double v = 0.0; for (int i = 0; i < nh; ++i) { const double d = z[(long)j * nh + i] - means[j]; v += d * d; }
    mv += v / (nh - 1.0); mm += means[j];
  }
  mv /= m; mm /= m;
  double vm = 0.0; for (int j = 0; j < m; ++j) vm += (means[j] - mm) * (means[j] - mm);
  vm /= (m - 1.0);
  const double rh = rhat_from(vm, mv, nh);
  if (ess) {
    const double vp = var_plus_of(vm, mv, nh);
    for (int j = 0; j < m; ++j) for (int i = 0; i < nh; ++i) z[(long)j * nh + i] -= means[j];
    auto acov = [&](int t) { double s = 0.0; for (int j = 0; j < m; ++j) for (int i = 0; i + t < nh; ++i) s += z[(long)j * nh + i] * z[(long)j * nh + i + t]; return s / ((double)m * nh); };
    if (!(vp > 0.0)) *ess = NAN;
    else {
      Geyer g; g.start(nh, rho_of(acov(1), mv, vp));
      while (g.wants()) { const int t = g.next(); g.feed(rho_of(acov(t), mv, vp), rho_of(acov(t + 1), mv, vp)); }
      *ess = g.ess((long)m * nh);
    }
  }
  delete[] means;
  return rh;
}
// ranks: optional [N] output of the average ranks of the split values (the CPU check compares them exactly)
inline void summary_column_host(const double* x, int M, int n, double* out, double* ranks = nullptr) {
  const long Mn = (long)M * n;
  const int nh = n / 2, m = 2 * M;
  const long N = (long)m * nh;
  for (int f = 0; f < SUM_FIELDS; ++f) out[f] = NAN;
  double s = 0.0; bool bad = false;
  for (long i = 0; i < Mn; ++i) { bad = bad || !isfinite(x[i]); s += x[i]; }
  if (bad || Mn < 1) return;
  const double mean = s / Mn;
  double ss = 0.0; for (long i = 0; i < Mn; ++i) ss += (x[i] - mean) * (x[i] - mean);
  out[SUM_MEAN] = mean; out[SUM_SD] = sqrt(ss / (Mn - 1.0));
  double* S = new double[Mn + 2 * (N > 0 ? N : 1)];
  double* Z = S + Mn;
  double* X = Z + (N > 0 ? N : 1);
  for (long i = 0; i < Mn; ++i) S[i] = x[i];
  summary_sort(S, Mn);
  out[SUM_Q05] = quantile7_sorted(S, Mn, 0.05); out[SUM_Q50] = quantile7_sorted(S, Mn, 0.5); out[SUM_Q95] = quantile7_sorted(S, Mn, 0.95);
  if (nh >= 2) {
    for (long k = 0; k < N; ++k) X[k] = x[split_source(k, nh, n)];
    for (long k = 0; k < N; ++k) S[k] = X[k];
    summary_sort(S, N);
    if (S[0] < S[N - 1]) {
      const double q05 = quantile7_sorted(S, N, 0.05), med = quantile7_sorted(S, N, 0.5), q95 = quantile7_sorted(S, N, 0.95);
      for (long k = 0; k < N; ++k) { const double r = average_rank(S, N, X[k]); if (ranks) ranks[k] = r; Z[k] = blom_z(r, N); }
      double eb = NAN;
      const double rb = summary_seq_host(Z, m, nh, &eb);
      for (long k = 0; k < N; ++k) S[k] = fabs(X[k] - med);
      summary_sort(S, N);
      for (long k = 0; k < N; ++k) Z[k] = blom_z(average_rank(S, N, fabs(X[k] - med)), N);
      const double rf = summary_seq_host(Z, m, nh, nullptr);
      double e05 = NAN, e95 = NAN;
      for (long k = 0; k < N; ++k) Z[k] = X[k] <= q05 ? 1.0 : 0.0;
      summary_seq_host(Z, m, nh, &e05);
      for (long k = 0; k < N; ++k) Z[k] = X[k] <= q95 ? 1.0 : 0.0;
      summary_seq_host(Z, m, nh, &e95);
      out[SUM_RHAT] = fmax(rb, rf);                     // a NaN side (no variance) gives way
      out[SUM_ESS_BULK] = eb;
      out[SUM_ESS_TAIL] = isnan(e05) ? e95 : (isnan(e95) ? e05 : (e05 < e95 ? e05 : e95));
    }
  }
  delete[] S;
}
#endif

}  // namespace ppcx
