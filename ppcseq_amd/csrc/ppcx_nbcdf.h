// ppcx_nbcdf.h -- the two tail probabilities of a negative binomial count, X ~ NB(mean mu = e^eta, size phi):
//   P(X <= k) = I_x(phi, k + 1),  x = phi / (phi + mu)      (the regularised incomplete beta function, A&S 26.5.24 / 6.6.2)
// by the continued fraction of I_x(a, b) (A&S 26.5.8; the even / odd coefficients of Numerical Recipes' betacf), evaluated on
// the side where it converges fast: in x where x < (a + 1) / (a + b + 2), else in 1 - x for 1 - I_x(a, b) = I_{1 - x}(b, a).
// That is the side of the smaller tail wherever the distribution has a body (the switch-over is near its mean), so a small tail
// is not formed as 1 - (nearly 1) there. Where nearly all the mass lies at 0 (phi << 1) the side in x can hold the larger tail
// at counts beyond the mean; the smaller one is then 1 - it, with the absolute error of the larger (1e-15).
//
// Shared by the gfx950 kernel (ppcx_ppc_exact.hip), the testing build (ppcx_testing_math.hip) and the CPU check
// (tests/ppc_exact_host): everything here is `__host__ __device__`.
//
// The prefactor. With a = phi, b = k + 1:  x^a (1 - x)^b / B(a, b) = pmf(k) (k + phi) (1 - x),  pmf the NB probability of k, so
//   I_x(a, b) = pmf(k) (k + phi) (1 - x) cf(a, b, x) / a,     1 - I_x(a, b) = pmf(k) (k + phi) (1 - x) cf(b, a, 1 - x) / b.
// log pmf(k) is formed from the pieces the log-likelihood uses (ppcx_disp.h, ppcx_math.h) -- the Stirling tails at k + phi and
// k + 1 and the Stirling excess of phi, the leading terms cancelled analytically -- and regrouped around the mean, so that no
// term is larger than |k - mu| (loo_ll's y eta - (y + phi) ln w carries terms of size y eta: 4e7 at y = 2.6e6, 4e-9 of the pmf):
//   k >= 8:  log pmf = M - ln((k + phi) (k + 1) / phi) / 2 + 1 - ln(2 pi) / 2 + lg_tail(1 / (k + phi)) - dlt(phi) - lg_tail(1 / (k + 1)),
//            M = (k + phi) ln((k + phi) / (phi + mu)) + k ln(mu / (k + 1))                                   (A: terms of size |k - mu|)
//              = k log1p((phi - 1) / (k + 1)) - k log1p(phi / mu) + phi ln((k + phi) / (phi + mu))            (B: terms of size phi)
//            B where phi < |k - mu|, else A; the logarithms of quotients by nb_log_ratio
//   k <  8:  log pmf = ln prod_{j < k} (1 + j / phi) + k ln phi - ln k! - phi log1p(mu / phi) - k log1p(phi / mu)   (exact recurrences)
//
// The continued fraction by the modified Lentz recurrence with ONE division per half-step and no transcendental in the loop: a
// coefficient N / D is never formed; with e = 1 / c, P = D + N e, Q = D + N d, t = 1 / (P Q):  e' = D Q t, d' = D P t and the
// factor of the step is P^2 t. It ends where a whole step changes the value by less than kNbCdfEps, and after kNbCdfMaxIter
// steps at the latest: a point that reaches the cap is NaN (the loop is bounded for every input).
#pragma once
#include "ppcx_math.h"
#include "ppcx_disp.h"

#ifndef PPCX_NO_CONTRACT
#if defined(__clang__)
#define PPCX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PPCX_NO_CONTRACT
#endif
#endif

namespace ppcx {

constexpr int kNbCdfMaxIter = 2048;            // steps (two half-steps each) of the continued fraction at most
constexpr double kNbCdfEps = 1e-15;            // relative change of a step at which it ends
constexpr double kNbCdfTiny = 1e-290;          // Lentz's guard of a vanishing denominator

// cf(a, b, x) of I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) cf(a, b, x); *iters the steps taken, kNbCdfMaxIter + 1: not converged (NaN)
PPCX_HD double nb_beta_cf(double a, double b, double x, int* iters) {
  PPCX_NO_CONTRACT
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double e = 1.0;                                                  // 1 / c
  double q0 = qap - qab * x;
  q0 = fabs(q0) < kNbCdfTiny ? kNbCdfTiny : q0;
  double d = qap / q0;
  double h = d;
  int m = 1;
  bool done = false;
  for (; m <= kNbCdfMaxIter; ++m) {
    const double dm = (double)m, a2 = a + 2.0 * dm;
    // even half-step: N / D = m (b - m) x / ((a + 2m - 1) (a + 2m))
    double N = dm * (b - dm) * x, D = (qam + 2.0 * dm) * a2;
    double P = D + N * e, Q = D + N * d;
    P = fabs(P) < kNbCdfTiny ? kNbCdfTiny : P;
    Q = fabs(Q) < kNbCdfTiny ? kNbCdfTiny : Q;
    double t = 1.0 / (P * Q);
    e = D * Q * t; d = D * P * t;
    h *= P * P * t;
    // odd half-step: N / D = -(a + m) (a + b + m) x / ((a + 2m) (a + 2m + 1))
    N = -(a + dm) * (qab + dm) * x; D = a2 * (qap + 2.0 * dm);
    P = D + N * e; Q = D + N * d;
    P = fabs(P) < kNbCdfTiny ? kNbCdfTiny : P;
    Q = fabs(Q) < kNbCdfTiny ? kNbCdfTiny : Q;
    t = 1.0 / (P * Q);
    e = D * Q * t; d = D * P * t;
    const double del = P * P * t;
    h *= del;
    if (fabs(del - 1.0) < kNbCdfEps) { done = true; break; }
  }
  *iters = done ? m : kNbCdfMaxIter + 1;
  return done ? h : NAN;
}

// ln(num / den) with dif = num - den given without cancellation: log1p of the small relative difference near 1 (where the
// quotient's rounding would be the whole result), the logarithm of the quotient elsewhere (where 1 + dif / den rounds away
// the quotient's low bits)
PPCX_HD double nb_log_ratio(double num, double den, double dif) {
  PPCX_NO_CONTRACT
  return fabs(dif) < 0.5 * den ? log1p(dif / den) : log(num / den);
}
// log pmf(k) of NB(mu, phi), ln phi given (the header comment); mu, phi finite and > 0
PPCX_HD double nb_log_pmf(int k, double mu, double phi, double lnphi) {
  PPCX_NO_CONTRACT
  const double kd = (double)k;
  if (k < 8) {
    double Pr = 1.0;
    const double invphi = 1.0 / phi;
    for (int j = 0; j < k; ++j) Pr *= fma((double)j, invphi, 1.0);
    const double tail = k > 0 ? kd * log1p(phi / mu) : 0.0;
    return log(Pr) + kd * lnphi - lgamma_int1(kd) - phi * log1p(mu * invphi) - tail;
  }
  double dlt, dps, lg1, lg2, dg;
  stirling_excess_acc(phi, lnphi, &dlt, &dps);
  const double xp = kd + phi, x1 = kd + 1.0;
  stirling_tails(1.0 / xp, &lg1, &dg);
  stirling_tails(1.0 / x1, &lg2, &dg);
  const double l1 = nb_log_ratio(xp, phi + mu, kd - mu);
  double main;
  if (phi < fabs(kd - mu)) main = (kd * log1p((phi - 1.0) / x1) - kd * log1p(phi / mu)) + phi * l1;      // form B
  else main = xp * l1 + kd * nb_log_ratio(mu, x1, mu - x1);                                              // form A
  const double t3 = 0.5 * (log(xp) + log(x1) - lnphi);
  return (main - t3) + (1.0 - 9.18938533204672742e-01) + ((lg1 - lg2) - dlt);
}

// le = P(X <= k), gt = P(X > k), pmf = P(X = k) of NB(mean e^eta, size phi), k >= 0; lnphi = ln phi. The smaller of le and gt
// -- the member on the side the header comment names -- comes from the continued fraction directly, the other is 1 - it. *iters: the steps of the continued fraction (0: none).
// Invalid parameters (nb2_invalid), or a continued fraction at its cap: all NaN.
PPCX_HD void nb2_cdf_pair(int k, double eta, double phi, double lnphi, double* le, double* gt, double* pmf, int* iters) {
  PPCX_NO_CONTRACT
  *iters = 0;
  if (nb2_invalid(eta, phi) || k < 0) { *le = *gt = *pmf = NAN; return; }
  const double mu = exp(eta);
  if (!(mu > 0.0)) { *le = 1.0; *gt = 0.0; *pmf = k == 0 ? 1.0 : 0.0; return; }      // e^eta underflowed: all mass at 0
  if (!isfinite(mu)) { *le = 0.0; *gt = 1.0; *pmf = 0.0; return; }                   // e^eta overflowed: no mass at any count
  const double kd = (double)k, a = phi, b = kd + 1.0;
  const double den = phi + mu, x = phi / den, x1 = mu / den;                         // x1 = 1 - x without the subtraction
  const double pm = exp(nb_log_pmf(k, mu, phi, lnphi));
  const double Bt = pm * (kd + phi) * x1;
  *pmf = pm;
  if (x < (a + 1.0) / (a + b + 2.0)) {
    const double v = Bt * nb_beta_cf(a, b, x, iters) / a;
    *le = v; *gt = 1.0 - v;
  } else {
    const double v = Bt * nb_beta_cf(b, a, x1, iters) / b;
    *gt = v; *le = 1.0 - v;
  }
}

// p_le = P(X <= y), p_ge = P(X >= y) = P(X > y) + P(X = y) (a sum of two positive terms where P(X > y) is the small side; 1 at
// y = 0). Returns the steps of the continued fraction.
PPCX_HD int nb2_log_tails_ln(int y, double eta, double phi, double lnphi, double* p_le, double* p_ge) {
  PPCX_NO_CONTRACT
  double le, gt, pm; int it;
  nb2_cdf_pair(y, eta, phi, lnphi, &le, &gt, &pm, &it);
  *p_le = le;
  *p_ge = y == 0 && !isnan(le) ? 1.0 : gt + pm;
  return it;
}
PPCX_HD int nb2_log_tails(int y, double eta, double phi, double* p_le, double* p_ge) {
  return nb2_log_tails_ln(y, eta, phi, log(phi), p_le, p_ge);
}

}  // namespace ppcx
