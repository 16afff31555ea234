// ppcx_psis.h -- the Pareto shape estimate k-hat of Pareto-smoothed importance sampling (ppcx_fit_psis): what rstan::vb
// (rstan >= 2.21) reports after an ADVI fit, through loo's psis(r, r_eff = NA) on the log ratios r = log_p - log_g of the
// output draws. Vehtari, Simpson, Gelman, Yao, Gabry (2024), "Pareto smoothed importance sampling", JMLR; the tail fit is
// Zhang and Stephens (2009), "A new and efficient estimation method for the generalized Pareto distribution", with loo's
// weakly informative prior.
//
// Shared by the gfx950 kernel (ppcx_psis.hip, one workgroup per column) and the CPU check (tests/psis_host): the building
// blocks below are `__host__ __device__`; psis_khat_host at the end is their sequential composition, which the CPU check
// runs, and the kernel composes the same blocks with workgroup-parallel loops.
//
// Spec of one column v[0 .. n):
//   a NaN or +Inf entry: NaN. Entries equal to -Inf take no part (a draw whose log density is not finite has log ratio -Inf;
//   rstan puts a large negative number there instead, which has the same effect on the tail fit); N = the other entries.
//   1. M = ceil(min(0.2 N, 3 sqrt(N))) (evaluated as written, in double). M < 5, or the M tail values all equal: +Inf.
//   2. sorted ascending and shifted by the largest value: the tail is the M largest values, the cutoff c the largest value
//      outside it (the (M + 1)-th largest); x_i = exp(tail_i) - exp(c), ascending.
//   3. loo's gpdfit: prior = 3, m = 30 + floor(sqrt(M)), x* = x[floor(M / 4 + 0.5)] (1-based),
//      theta_j = 1 / x_M + (1 - sqrt(m / (j - 1/2))) / prior / x*, j = 1 .. m;
//      k_j = mean_i log1p(-theta_j x_i), l_j = M (log(-theta_j / k_j) - k_j - 1);
//      w = softmax(l); weights below 10 DBL_EPSILON are dropped and the rest renormalised; theta^ = sum_j w_j theta_j;
//      k = mean_i log1p(-theta^ x_i).
//   4. k-hat = (M k + 5) / (M + 10); NaN: +Inf.
// The per-parameter k-hat of rstan's summary is the same procedure on 1/2 log1p(theta_d^2) + r for draw column d.
#pragma once
#include <stdint.h>
#include "ppcx_math.h"

#if defined(__clang__) && !defined(PPCX_NO_CONTRACT)
#define PPCX_NO_CONTRACT _Pragma("clang fp contract(off)")
#elif !defined(PPCX_NO_CONTRACT)
#define PPCX_NO_CONTRACT
#endif

namespace ppcx {

constexpr double kPsisPrior = 3.0;
constexpr double kPsisMinWeight = 10.0 * 2.220446049250313e-16;   // 10 DBL_EPSILON

// tail length M of N finite values (step 1); PSIS-LOO divides N by the relative efficiency r_eff of the cell's draws
// (ppcx_loo.h step 1; N / 1.0 is N: the same bits)
PPCX_HD int psis_tail_len(long N, double r_eff = 1.0) {
  const double a = 0.2 * (double)N, b = 3.0 * sqrt((double)N / r_eff);
  return (int)ceil(a < b ? a : b);
}
// grid size m of the profile fit (step 3)
PPCX_HD int psis_grid_size(int M) { return 30 + (int)floor(sqrt((double)M)); }
// 1-based index of x* in the ascending x[1 .. M]
PPCX_HD int psis_xstar_index(int M) { return (int)floor((double)M / 4.0 + 0.5); }
// grid point theta_j, j = 1 .. m
PPCX_HD double psis_theta(int j, int m, double x_max, double xstar) {
  PPCX_NO_CONTRACT
  const double s = sqrt((double)m / ((double)j - 0.5));
  return 1.0 / x_max + (1.0 - s) / kPsisPrior / xstar;
}
// profile log-likelihood l_j of theta_j, given k_j = mean_i log1p(-theta_j x_i)
PPCX_HD double psis_ell(double theta, double k, int M) {
  PPCX_NO_CONTRACT
  return (double)M * (log(-theta / k) - k - 1.0);
}
// theta^ from the m grid points (sequential, fixed order): softmax of l, weights below kPsisMinWeight dropped, renormalised.
// A NaN l_j makes theta^ NaN (and k-hat +Inf), as in loo.
PPCX_HD double psis_theta_hat(const double* theta, const double* ell, int m) {
  PPCX_NO_CONTRACT
  double mx = ell[0];
  for (int j = 1; j < m; ++j) mx = (ell[j] > mx || isnan(ell[j])) ? ell[j] : mx;
  double s = 0.0;
  for (int j = 0; j < m; ++j) s += exp(ell[j] - mx);
  double ws = 0.0, th = 0.0;
  for (int j = 0; j < m; ++j) {
    const double w = exp(ell[j] - mx) / s;
    if (w < kPsisMinWeight) continue;
    ws += w; th += w * theta[j];
  }
  return th / ws;
}
// step 4: the weakly informative adjustment of the mean k = (sum_i log1p(-theta^ x_i)) / M
PPCX_HD double psis_adjust(double k, int M) {
  PPCX_NO_CONTRACT
  const double kh = ((double)M * k + 5.0) / ((double)M + 10.0);
  return isnan(kh) ? INFINITY : kh;
}
// order-preserving map of a double (not NaN) to an unsigned key and back: a < b <=> key(a) < key(b); -0 sorts below +0
PPCX_HD uint64_t psis_key(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
PPCX_HD double psis_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}
// value of draw i of column col: the log ratio itself (col < 0) or 1/2 log1p(theta^2) + r
PPCX_HD double psis_value(double theta, double r, int col) {
  PPCX_NO_CONTRACT
  return col < 0 ? r : 0.5 * log1p(theta * theta) + r;
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
namespace ppcx {
// steps 2 and 3 for the CPU checks, sequentially: the ascending s[0 .. N) (no NaN, all finite) with M (5 <= M < N) of them
// in a tail that is not all equal -> the mean k before the prior adjustment, theta^ and exp(cutoff - largest)
struct PsisTailHost { double k_mean, theta_hat, ec; };
inline PsisTailHost psis_tail_host(const double* s, long N, int M) {
  const double mx = s[N - 1], c = s[N - M - 1];
  std::vector<double> x(M);
  const double ec = exp(c - mx);
  for (int i = 0; i < M; ++i) x[i] = exp(s[N - M + i] - mx) - ec;
  const int m = psis_grid_size(M);
  const double xstar = x[psis_xstar_index(M) - 1];
  std::vector<double> th(m), ll(m);
  for (int j = 0; j < m; ++j) {
    th[j] = psis_theta(j + 1, m, x[M - 1], xstar);
    double a = 0.0;
    for (int i = 0; i < M; ++i) a += log1p(-th[j] * x[i]);
    ll[j] = psis_ell(th[j], a / M, M);
  }
  const double t = psis_theta_hat(th.data(), ll.data(), m);
  double a = 0.0;
  for (int i = 0; i < M; ++i) a += log1p(-t * x[i]);
  return PsisTailHost{a / M, t, ec};
}
// the whole spec, sequentially, for the CPU check
inline double psis_khat_host(const double* v, long n) {
  std::vector<double> s;
  s.reserve((size_t)n);
  for (long i = 0; i < n; ++i) {
    if (isnan(v[i]) || v[i] == INFINITY) return NAN;
    if (v[i] != -INFINITY) s.push_back(v[i]);
  }
  const long N = (long)s.size();
  const int M = psis_tail_len(N);
  if (M < 5 || M >= N) return INFINITY;
  std::sort(s.begin(), s.end());
  if (s[N - M] == s[N - 1]) return INFINITY;
  return psis_adjust(psis_tail_host(s.data(), N, M).k_mean, M);
}
}  // namespace ppcx
#endif
