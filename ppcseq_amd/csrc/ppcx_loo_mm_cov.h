// ppcx_loo_mm_cov.h -- gene-local moment matching with the covariance step (ppcx_fit_loo_moment_match_cov): the third
// transformation of Paananen, Piironen, Buerkner, Vehtari (2021), "Implicitly adaptive importance sampling" (loo's
// shift_and_cov), beside the shift and the shift with a per-coordinate scale of ppcx_loo_mm.h, and the split transformation of
// ppcx_loo_mm_split.h on the affine map that results. Restated from the paper and the published package; not run against R.
//
// Why. A gene's coordinates are correlated by construction: the intercept and the slopes share every sample's linear predictor
// and sigma_raw is tied to the intercept through its prior. An outlying cell in one factor level moves the posterior along a
// direction that no per-coordinate scale can follow. loo transforms all D coordinates, so its weighted covariance is noise;
// here the matrix is d x d with d = 2 .. C + 1 <= 17, estimated from all n draws and factorised by one thread.
//
// Shared by the gfx950 kernel (ppcx_loo_mm_cov.hip) and the CPU check (tests/loo_mm_cov_twin): the blocks below are
// `__host__ __device__`; loo_mm_cov_cell_host at the end is their sequential composition. The local density, the prior, eta and
// the cell's log-likelihood of ppcx_loo_mm.h are restated here against the general state; ppcx_loo_mm.h's own are untouched.
//
// One cell (g, s) from what ppcx_loo_mm.h reads:
//   1. The state: an affine map (M [nc][nc] row-major, b [nc]), nc = C + 1, initially the identity. The current draws are
//      t_i = M theta_i + b, formed from the table where they are needed, never stored: row c is the sum over the gene's
//      coordinates k in ascending order of M[c][k] theta_ik, then + b[c], with contraction off. A row or column that is no
//      coordinate of the gene (loo_mm_is_coord false) stays the identity's with shift 0: such a row of t is the table's.
//   2. Steps 0, 1 and 4 and the loop's gates are ppcx_loo_mm.h's: the finished cells, Q0, the strict k' < k, the tail length from
//      the participating draws and r_eff, the tie rule, ratios that are not finite to -Inf, the constant Jacobian.
//   3. Per iteration the moments m, v, mw, vw of every coordinate of the current t, as ppcx_loo_mm.h step 3 forms them: the same
//      formulas and the same two sweeps.
//   4. Candidate 1 (shift): b' = b + (mw - m). Candidate 2 (shift and scale): s = sqrt(vw / v), M' = diag(s) M,
//      b' = s (b - m) + mw; invalid unless every s is finite and > 0.
//   5. Candidate 3 (shift and covariance), tried when 1 is refused and 2 is refused or invalid. Over the gene's d coordinates
//        Sigma   = sum_i (t_i - m)(t_i - m)^T / (n - 1),
//        Sigma_w = sum_i w_i (t_i - mw)(t_i - mw)^T / (1 - sum w_i^2)      (the unbiased form of R's stats::cov.wt),
//      both centred, in a sweep after the means; the pairs (a <= b) in ascending row-major order, each pair one sum over the
//      draws. Lower Cholesky factors L, L_w. The candidate is invalid when n <= d, when 1 - sum w^2 is not positive or not
//      finite, or when a pivot of either factor is not finite or <= 0: a refusal, never a state. The pivot of a singular matrix
//      is rounding noise of either sign, so a pivot that is not above kLooMmCovPivot (1e-12) times its own diagonal entry counts
//      as <= 0: a duplicated coordinate is refused on every machine. Otherwise Tm = L_w L^-1 by substitution, M' = Tm M,
//      b' = Tm (b - m) + mw, so that Tm Sigma Tm^T = Sigma_w.
//   6. The inverse is carried along the accepted steps, for the split; this accumulated form is the definition. Shift:
//      unchanged. Scale: Minv' = Minv diag(1 / s), logJ += sum log s. Covariance: Minv' = Minv (L L_w^-1),
//      logJ += sum log L_w,jj - sum log L_jj. At the end binv = -Minv b.
//   7. split: steps 2 - 7 of ppcx_loo_mm_split.h with the three states (M, b), the identity and (Minv, binv) and this logJ. The
//      first n / 2 draws in the fit's order are transformed; khat stays the matching's; khat_split is a diagnostic. A cell with
//      iterations == 0 is not split.
//   8. The record, loo_mm_cov_fields(C) = 9 + (C + 1)(C + 1) + (C + 1): elpd_loo, p_loo, looic, khat, khat_before, iterations,
//      cov_iterations (the accepted steps of kind 3), elpd_loo_matched (the unsplit estimate; elpd_loo without split),
//      khat_split (NaN without split or with iterations == 0), transform [C + 1][C + 1] row-major, shift [C + 1]. A cell with
//      iterations == 0 holds ppcx_fit_loo's four fields bit for bit, the identity and zeros.
// Still left out: the exact predictive under covariance-matched weights, mcse / n_eff of a matched cell, ADVI fits.
// Every reduction runs in a fixed order with contraction off: a cell's fields depend on its own gene's data only.
#pragma once
#include <stdint.h>
#include "ppcx_loo_mm.h"
#include "ppcx_loo_mm_split.h"

namespace ppcx {

constexpr int kLooMmCovHead = 9;               // the six of ppcx_loo_mm.h, cov_iterations, elpd_loo_matched, khat_split
constexpr int kLooMmCovNc = kMaxC + 1;         // the largest nc
constexpr double kLooMmCovPivot = 1e-12;       // a Cholesky pivot at or below this fraction of its diagonal entry: singular
PPCX_HD int loo_mm_cov_fields(int C) { return kLooMmCovHead + (C + 1) * (C + 1) + (C + 1); }   // PPCX_LOO_MM_COV_FIELDS(C)

// the gene's d coordinates among the table's rows, ascending
PPCX_HD int loo_mm_cov_dim(const LooMmGene& g) { return g.checked ? g.C + 1 : 2; }
PPCX_HD int loo_mm_cov_row(const LooMmGene& g, int a) { return g.checked ? a : (a == 0 ? 0 : g.C); }

// step 1: the identity
PPCX_HD void loo_mm_cov_identity(double* M, double* b, int nc) {
  for (int r = 0; r < nc; ++r) {
    for (int c = 0; c < nc; ++c) M[r * nc + c] = r == c ? 1.0 : 0.0;
    if (b) b[r] = 0.0;
  }
}
// coordinate c of draw i under the state
PPCX_HD double loo_mm_cov_coord(const LooMmGene& g, int c, long i, const double* M, const double* b) {
  PPCX_NO_CONTRACT
  if (!loo_mm_is_coord(g, c)) return g.Tg[(long)c * g.n + i];
  const int nc = g.C + 1, d = loo_mm_cov_dim(g);
  double t = 0.0;
  for (int a = 0; a < d; ++a) { const int k = loo_mm_cov_row(g, a); t += M[c * nc + k] * g.Tg[(long)k * g.n + i]; }
  return t + b[c];
}
// every row of draw i under the state: t [C + 1]
PPCX_HD void loo_mm_cov_point(const LooMmGene& g, long i, const double* M, const double* b, double* t) {
  PPCX_NO_CONTRACT
  const int nc = g.C + 1, d = loo_mm_cov_dim(g);
  double th[kLooMmCovNc];
  for (int c = 0; c < nc; ++c) th[c] = g.Tg[(long)c * g.n + i];
  for (int c = 0; c < nc; ++c) {
    if (!loo_mm_is_coord(g, c)) { t[c] = th[c]; continue; }
    double x = 0.0;
    for (int a = 0; a < d; ++a) { const int k = loo_mm_cov_row(g, a); x += M[c * nc + k] * th[k]; }
    t[c] = x + b[c];
  }
}
// linear predictor of sample s at the point t
PPCX_HD double loo_mm_cov_eta(const LooMmGene& g, int s, const double* t) {
  PPCX_NO_CONTRACT
  double eta = g.expo[s] + g.X[s] * t[0];
  for (int c = 1; c < g.C; ++c) eta += g.X[(long)c * g.S + s] * t[c];
  return eta;
}
// the gene's prior terms at draw i's hyper-parameters and the point t (ppcx_loo_mm.h step 1)
PPCX_HD double loo_mm_cov_prior(const LooMmGene& g, long i, const double* t) {
  PPCX_NO_CONTRACT
  double u6[6];
  for (int k = 0; k < 6; ++k) u6[k] = g.U[(long)k * g.n + i];
  const Hyper h = make_hyper(u6, g.lambda_mu_mu);
  const double t0 = t[0], sg = t[g.C];
  const double z = (t0 - h.xi) * h.inv_om;
  double lerfc, ratio;
  log_erfc_and_ratio(-h.lambda_skew * z * 0.70710678118654752440, &lerfc, &ratio);
  double lp = -0.5 * z * z + lerfc;
  const double r = sg - (h.sigma_slope * t0 + h.sigma_intercept);
  lp += -0.5 * r * (r * h.inv_ss2);
  if (g.checked) {
    for (int c = 1; c < g.C; ++c) {
      const double al = t[c];
      lp += c == 1 ? -fabs(al) : -(al * al) / 12.5;
    }
  }
  return lp;
}
// q(t_i; h_i) under the state, and the log-likelihood of the cell of sample s_cell itself (whether excluded or not)
PPCX_HD double loo_mm_cov_density(const LooMmGene& g, long i, const double* M, const double* b, int s_cell, double* ll_cell) {
  PPCX_NO_CONTRACT
  double t[kLooMmCovNc];
  loo_mm_cov_point(g, i, M, b, t);
  const double sg = t[g.C];
  const DispPoint p = disp_point(sg);
  double q = 0.0;
  for (int s = 0; s < g.S; ++s) {
    const int ye = g.yrow[s];
    if (ye < 0 && s != s_cell) continue;
    const double ll = loo_mm_ll(ye < 0 ? -ye - 1 : ye, loo_mm_cov_eta(g, s, t), sg, p);
    if (ye >= 0) q += ll;
    if (s == s_cell) *ll_cell = ll;
  }
  return q + loo_mm_cov_prior(g, i, t);
}
// the log-likelihood of the cell of sample s alone, under the state
PPCX_HD double loo_mm_cov_cell_ll(const LooMmGene& g, long i, const double* M, const double* b, int s) {
  PPCX_NO_CONTRACT
  double t[kLooMmCovNc];
  loo_mm_cov_point(g, i, M, b, t);
  const int ye = g.yrow[s];
  return loo_mm_ll(ye < 0 ? -ye - 1 : ye, loo_mm_cov_eta(g, s, t), t[g.C], disp_point(t[g.C]));
}

// step 4: candidates 1 and 2 from the moments m, mw and the scales sc (rows of the table; read at the gene's coordinates only)
PPCX_HD void loo_mm_cov_cand12(const LooMmGene& g, const double* M, const double* b, const double* m, const double* mw, const double* sc,
                               double* b1, double* M2, double* b2) {
  PPCX_NO_CONTRACT
  const int nc = g.C + 1;
  for (int c = 0; c < nc; ++c) {
    const bool coord = loo_mm_is_coord(g, c);
    b1[c] = coord ? loo_mm_shift(b[c], m[c], mw[c]) : b[c];
    b2[c] = coord ? loo_mm_scaled_B(sc[c], b[c], m[c], mw[c]) : b[c];
    for (int k = 0; k < nc; ++k) M2[c * nc + k] = coord ? loo_mm_scaled_A(sc[c], M[c * nc + k]) : M[c * nc + k];
  }
}

// lower Cholesky factor of the d x d matrix whose lower triangle A holds (stride nc), in place; false at a pivot that is not
// finite, <= 0 or not above kLooMmCovPivot of its diagonal entry
PPCX_HD bool loo_mm_cov_chol(double* A, int d, int nc) {
  PPCX_NO_CONTRACT
  for (int j = 0; j < d; ++j) {
    const double ajj = A[j * nc + j];
    double p = ajj;
    for (int k = 0; k < j; ++k) p -= A[j * nc + k] * A[j * nc + k];
    if (!(isfinite(p) && p > 0.0 && p > kLooMmCovPivot * ajj)) return false;
    const double l = sqrt(p);
    A[j * nc + j] = l;
    for (int r = j + 1; r < d; ++r) {
      double x = A[r * nc + j];
      for (int k = 0; k < j; ++k) x -= A[r * nc + k] * A[j * nc + k];
      A[r * nc + j] = x / l;
    }
  }
  return true;
}
// X = P Q^-1 for lower triangular P, Q (d x d, stride nc), lower triangular: row r from X Q = P, column j = r down to 0
PPCX_HD void loo_mm_cov_tri_right_div(const double* P, const double* Q, int d, int nc, double* X) {
  PPCX_NO_CONTRACT
  for (int r = 0; r < d; ++r) {
    for (int j = d - 1; j > r; --j) X[r * nc + j] = 0.0;
    for (int j = r; j >= 0; --j) {
      double x = P[r * nc + j];
      for (int k = j + 1; k <= r; ++k) x -= X[r * nc + k] * Q[k * nc + j];
      X[r * nc + j] = x / Q[j * nc + j];
    }
  }
}
// step 5: candidate 3. SA, SB: the centred sums of the pairs in their lower triangles ([b][a], a <= b, stride nc, compact over
// the gene's coordinates); on return L and L_w. sw2 = sum w^2. Tm, Tinv: compact d x d (stride nc): L_w L^-1 and L L_w^-1.
// Returns whether the candidate is valid; then M3, b3 hold it and *dlogJ its log Jacobian.
PPCX_HD bool loo_mm_cov_cand3(const LooMmGene& g, double sw2, const double* m, const double* mw, double* SA, double* SB,
                              const double* M, const double* b, double* Tm, double* Tinv, double* M3, double* b3, double* dlogJ) {
  PPCX_NO_CONTRACT
  const int nc = g.C + 1, d = loo_mm_cov_dim(g);
  const long n = g.n;
  if (!(n > (long)d)) return false;
  const double den = 1.0 - sw2;
  if (!(isfinite(den) && den > 0.0)) return false;
  for (int r = 0; r < d; ++r)
    for (int c = 0; c <= r; ++c) { SA[r * nc + c] = SA[r * nc + c] / (double)(n - 1); SB[r * nc + c] = SB[r * nc + c] / den; }
  if (!loo_mm_cov_chol(SA, d, nc)) return false;
  if (!loo_mm_cov_chol(SB, d, nc)) return false;
  loo_mm_cov_tri_right_div(SB, SA, d, nc, Tm);
  loo_mm_cov_tri_right_div(SA, SB, d, nc, Tinv);
  double lw = 0.0, l0 = 0.0;
  for (int j = 0; j < d; ++j) { lw += log(SB[j * nc + j]); l0 += log(SA[j * nc + j]); }
  *dlogJ = lw - l0;
  for (int j = 0; j < nc * nc; ++j) M3[j] = M[j];
  for (int c = 0; c < nc; ++c) b3[c] = b[c];
  for (int a = 0; a < d; ++a) {
    const int ra = loo_mm_cov_row(g, a);
    for (int k = 0; k < d; ++k) {
      const int rk = loo_mm_cov_row(g, k);
      double x = 0.0;
      for (int j = 0; j <= a; ++j) x += Tm[a * nc + j] * M[loo_mm_cov_row(g, j) * nc + rk];
      M3[ra * nc + rk] = x;
    }
    double y = 0.0;
    for (int j = 0; j <= a; ++j) { const int rj = loo_mm_cov_row(g, j); y += Tm[a * nc + j] * (b[rj] - m[rj]); }
    b3[ra] = y + mw[ra];
  }
  return true;
}
// step 6: the inverse and the log Jacobian after an accepted step of `kind` (sc: candidate 2's scales; Tinv, dlogJ: candidate 3's)
PPCX_HD void loo_mm_cov_accept_inverse(const LooMmGene& g, int kind, const double* sc, const double* Tinv, double dlogJ, double* Minv,
                                       double* logJ) {
  PPCX_NO_CONTRACT
  const int nc = g.C + 1, d = loo_mm_cov_dim(g);
  if (kind == 2) {
    double lj = 0.0;
    for (int a = 0; a < d; ++a) {
      const int ra = loo_mm_cov_row(g, a);
      for (int k = 0; k < d; ++k) { const int rk = loo_mm_cov_row(g, k); Minv[ra * nc + rk] = Minv[ra * nc + rk] / sc[rk]; }
      lj += log(sc[ra]);
    }
    *logJ += lj;
  } else if (kind == 3) {
    for (int a = 0; a < d; ++a) {
      const int ra = loo_mm_cov_row(g, a);
      double row[kLooMmCovNc];
      for (int k = 0; k < d; ++k) {
        double x = 0.0;
        for (int j = k; j < d; ++j) x += Minv[ra * nc + loo_mm_cov_row(g, j)] * Tinv[j * nc + k];
        row[k] = x;
      }
      for (int k = 0; k < d; ++k) Minv[ra * nc + loo_mm_cov_row(g, k)] = row[k];
    }
    *logJ += dlogJ;
  }
}
// binv = -Minv b
PPCX_HD void loo_mm_cov_binv(const LooMmGene& g, const double* Minv, const double* b, double* binv) {
  PPCX_NO_CONTRACT
  const int nc = g.C + 1, d = loo_mm_cov_dim(g);
  for (int c = 0; c < nc; ++c) binv[c] = 0.0;
  for (int a = 0; a < d; ++a) {
    const int ra = loo_mm_cov_row(g, a);
    double x = 0.0;
    for (int j = 0; j < d; ++j) { const int rj = loo_mm_cov_row(g, j); x += Minv[ra * nc + rj] * b[rj]; }
    binv[ra] = -x;
  }
}
// step 7: the split's ratio of draw i (ppcx_loo_mm_split.h steps 3 - 5) under general states
PPCX_HD double loo_mm_cov_split_ratio(const LooMmGene& g, long i, const double* Mx, const double* bx, const double* Mi, const double* bi,
                                      double logJ, int s, double* ll_x) {
  PPCX_NO_CONTRACT
  double l, li;
  const double qx = loo_mm_cov_density(g, i, Mx, bx, s, &l);
  const double qinv = loo_mm_cov_density(g, i, Mi, bi, s, &li);
  const double dd = qinv - logJ;
  const double r = qx - l - loo_mm_split_logaddexp(qx, dd);
  *ll_x = l;
  return isfinite(r) ? r : -INFINITY;
}
// step 8: the record. M null: the identity and zeros. elpd_loo_matched = elpd_loo and khat_split = NaN until a cell is split.
PPCX_HD void loo_mm_cov_store(double* o, int C, double elpd, double p_loo, double looic, double khat, double khat_before, int iterations,
                              int cov_iterations, const double* M, const double* b) {
  const int nc = C + 1;
  o[0] = elpd; o[1] = p_loo; o[2] = looic; o[3] = khat; o[4] = khat_before; o[5] = (double)iterations; o[6] = (double)cov_iterations;
  o[7] = elpd; o[8] = NAN;
  for (int r = 0; r < nc; ++r) {
    for (int c = 0; c < nc; ++c) o[kLooMmCovHead + r * nc + c] = M ? M[r * nc + c] : (r == c ? 1.0 : 0.0);
    o[kLooMmCovHead + nc * nc + r] = b ? b[r] : 0.0;
  }
}
PPCX_HD void loo_mm_cov_store_split(double* o, double elpd, double lpd, double khat_split) {
  PPCX_NO_CONTRACT
  o[0] = elpd; o[1] = lpd - elpd; o[2] = -2.0 * elpd; o[8] = khat_split;
}
PPCX_HD void loo_mm_cov_store_split_nan(double* o) { o[0] = o[1] = o[2] = NAN; o[8] = NAN; }

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
namespace ppcx {
// the whole spec for one cell, sequentially, for the CPU check: out[loo_mm_cov_fields(C)]. kinds (may be null): the accepted
// candidates in order, 1, 2 or 3. inv (may be null): Minv [nc][nc], binv [nc] and logJ of the final state, nc nc + nc + 1 doubles.
inline void loo_mm_cov_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, bool split, double* out,
                                 std::vector<int>* kinds = nullptr, double* inv = nullptr) {
  PPCX_NO_CONTRACT
  const long n = g.n;
  const int C = g.C, nc = C + 1, d = loo_mm_cov_dim(g);
  std::vector<double> M(nc * nc), b(nc), Minv(nc * nc), binv(nc, 0.0), I(nc * nc), zero(nc, 0.0);
  loo_mm_cov_identity(M.data(), b.data(), nc);
  loo_mm_cov_identity(Minv.data(), nullptr, nc);
  loo_mm_cov_identity(I.data(), nullptr, nc);
  double logJ = 0.0;
  auto give_inverse = [&]() {
    if (!inv) return;
    for (int j = 0; j < nc * nc; ++j) inv[j] = Minv[j];
    for (int c = 0; c < nc; ++c) inv[nc * nc + c] = binv[c];
    inv[nc * nc + nc] = logJ;
  };
  const bool excluded = g.yrow[s] < 0;
  if (kinds) kinds->clear();
  give_inverse();
  // ---- step 0 of ppcx_loo_mm.h
  std::vector<double> ll(n);
  for (long i = 0; i < n; ++i) ll[i] = loo_mm_cov_cell_ll(g, i, M.data(), b.data(), s);
  double loo4[kLooFields];
  loo_cell_host(ll.data(), n, r_eff, excluded, loo4);
  loo_mm_cov_store(out, C, loo4[0], loo4[1], loo4[2], loo4[3], loo4[3], 0, 0, nullptr, nullptr);
  if (loo_mm_finished(excluded, loo4[3], k_threshold, max_iters)) return;
  std::vector<double> r(n), lw;
  for (long i = 0; i < n; ++i) r[i] = -ll[i];
  double lpd;
  if (!loo_mm_lpd_host(ll, &lpd)) return;
  double k = loo_mm_psis_host(r, r_eff, lw);
  // ---- Q0 at the original draws
  std::vector<double> Q0(n);
  for (long i = 0; i < n; ++i) { double l; Q0[i] = loo_mm_cov_density(g, i, M.data(), b.data(), s, &l); }
  // ---- the loop
  int iters = 0, cov_iters = 0;
  std::vector<double> m(nc, 0.0), mw(nc, 0.0), sc(nc, 1.0), b1(nc), M2(nc * nc), b2(nc), M3(nc * nc), b3(nc), SA(nc * nc), SB(nc * nc),
      Tm(nc * nc), Tinv(nc * nc), lw2, w(n);
  while (k > k_threshold && iters < max_iters) {
    const double lse = loo_logsumexp_host(lw);
    bool ok2 = true;
    for (int c = 0; c < nc; ++c) {
      if (!loo_mm_is_coord(g, c)) continue;
      double st = 0.0, swt = 0.0, swt2 = 0.0, sd2 = 0.0;
      for (long i = 0; i < n; ++i) {
        const double t = loo_mm_cov_coord(g, c, i, M.data(), b.data()), wi = exp(lw[i] - lse);
        st += t; swt += wi * t; swt2 += wi * (t * t);
      }
      m[c] = loo_mm_mean(st, n);
      for (long i = 0; i < n; ++i) { const double dd = loo_mm_cov_coord(g, c, i, M.data(), b.data()) - m[c]; sd2 += dd * dd; }
      mw[c] = swt;
      sc[c] = loo_mm_scale(loo_mm_wvar(swt2, swt), loo_mm_var(sd2, n));
      ok2 = ok2 && loo_mm_scale_ok(sc[c]);
    }
    loo_mm_cov_cand12(g, M.data(), b.data(), m.data(), mw.data(), sc.data(), b1.data(), M2.data(), b2.data());
    int kind = 0;
    double dlogJ = 0.0;
    for (int cand = 1; cand <= 3 && !kind; ++cand) {
      if (cand == 2 && !ok2) continue;
      if (cand == 3) {
        double sw2 = 0.0;
        for (long i = 0; i < n; ++i) { w[i] = exp(lw[i] - lse); sw2 += w[i] * w[i]; }
        for (int a = 0; a < d; ++a)
          for (int c2 = a; c2 < d; ++c2) {
            const int ra = loo_mm_cov_row(g, a), rb = loo_mm_cov_row(g, c2);
            double sa = 0.0, sb = 0.0;
            for (long i = 0; i < n; ++i) {
              const double ta = loo_mm_cov_coord(g, ra, i, M.data(), b.data()), tb = loo_mm_cov_coord(g, rb, i, M.data(), b.data());
              sa += (ta - m[ra]) * (tb - m[rb]);
              sb += w[i] * ((ta - mw[ra]) * (tb - mw[rb]));
            }
            SA[c2 * nc + a] = sa; SB[c2 * nc + a] = sb;
          }
        if (!loo_mm_cov_cand3(g, sw2, m.data(), mw.data(), SA.data(), SB.data(), M.data(), b.data(), Tm.data(), Tinv.data(), M3.data(),
                              b3.data(), &dlogJ))
          break;
      }
      const double* Mc = cand == 1 ? M.data() : cand == 2 ? M2.data() : M3.data();
      const double* bc = cand == 1 ? b1.data() : cand == 2 ? b2.data() : b3.data();
      for (long i = 0; i < n; ++i) { double l; const double q = loo_mm_cov_density(g, i, Mc, bc, s, &l); r[i] = loo_mm_ratio(q, Q0[i], l); }
      const double k2 = loo_mm_psis_host(r, r_eff, lw2);
      if (k2 < k) {
        kind = cand; k = k2; lw = lw2;
        loo_mm_cov_accept_inverse(g, kind, sc.data(), Tinv.data(), dlogJ, Minv.data(), &logJ);
        const std::vector<double> Mn(Mc, Mc + nc * nc), bn(bc, bc + nc);
        M = Mn; b = bn;
      }
    }
    if (!kind) break;
    ++iters;
    cov_iters += kind == 3;
    if (kinds) kinds->push_back(kind);
  }
  if (iters == 0) return;
  // ---- step 4 of ppcx_loo_mm.h
  std::vector<double> a1, a2;
  for (long i = 0; i < n; ++i)
    if (lw[i] != -INFINITY) { a1.push_back(lw[i] + loo_mm_cov_cell_ll(g, i, M.data(), b.data(), s)); a2.push_back(lw[i]); }
  const double elpd = loo_logsumexp_host(a1) - loo_logsumexp_host(a2);
  loo_mm_cov_store(out, C, elpd, lpd - elpd, -2.0 * elpd, k, loo4[3], iters, cov_iters, M.data(), b.data());
  loo_mm_cov_binv(g, Minv.data(), b.data(), binv.data());
  give_inverse();
  if (!split) return;
  // ---- step 7
  const long h = loo_mm_split_half(n);
  std::vector<double> lx(n);
  bool any = false;
  for (long i = 0; i < n; ++i) {
    const bool first = i < h;
    r[i] = loo_mm_cov_split_ratio(g, i, first ? M.data() : I.data(), first ? b.data() : zero.data(), first ? I.data() : Minv.data(),
                                  first ? zero.data() : binv.data(), logJ, s, &lx[i]);
    any = any || r[i] != -INFINITY;
  }
  const double khat_split = loo_mm_psis_host(r, r_eff, lw);
  if (!any) { loo_mm_cov_store_split_nan(out); return; }
  a1.clear(); a2.clear();
  for (long i = 0; i < n; ++i) if (lw[i] != -INFINITY) { a1.push_back(lw[i] + lx[i]); a2.push_back(lw[i]); }
  loo_mm_cov_store_split(out, loo_logsumexp_host(a1) - loo_logsumexp_host(a2), lpd, khat_split);
}
}  // namespace ppcx
#endif
