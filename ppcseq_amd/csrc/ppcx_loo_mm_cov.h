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
// `__host__ __device__`; loo_mm_cov_cell_host at the end is their sequential composition. The local density, the moment sweeps and
// the sequential cell (steps 0 - 4, the gates, the accepts) are ppcx_loo_mm.h's, stated there once; this header gives them the affine state
// (LooMmAffine, whose point is loo_mm_cov_point's array) and its policy (LooMmCovCell: the candidates, step 5, the inverse).
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
// The exact predictive under these weights is ppcx_loo_mm_cov_exact.h, which reads this record and the accumulated inverse.
// Still left out: mcse / n_eff of a matched cell, ADVI fits.
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
// The affine state as ppcx_loo_mm.h's density and moment sweeps read one: a point is a private array filled once per draw
struct LooMmAffine {
  const double* M; const double* b;
  struct Point {
    double t[kLooMmCovNc];
    PPCX_HD double operator()(int c) const { return t[c]; }
  };
  PPCX_HD double coord(const LooMmGene& g, int c, long i) const { return loo_mm_cov_coord(g, c, i, M, b); }
  PPCX_HD Point point(const LooMmGene& g, long i) const { Point p; loo_mm_cov_point(g, i, M, b, p.t); return p; }
};

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

// ---- the affine state as the policy of ppcx_loo_mm.h's sequential cell. What a cell keeps beside the draws' arrays: the state (M, b), the
// three candidates, the accumulated inverse, the factors and the moments (the kernel's static LDS; eight (C + 1)^2 matrices at kMaxC)
constexpr int kCovNN = kLooMmCovNc * kLooMmCovNc;
struct LooMmCovShared {
  double M[kCovNN], M2[kCovNN], M3[kCovNN], Minv[kCovNN], Tinv[kCovNN], SA[kCovNN], SB[kCovNN], Tm[kCovNN];
  double b[kLooMmCovNc], b1[kLooMmCovNc], b2[kLooMmCovNc], b3[kLooMmCovNc], binv[kLooMmCovNc];
  double m[kLooMmCovNc], mw[kLooMmCovNc], sc[kLooMmCovNc];
  double logJ, dlogJ;
  int ok3;
};
struct LooMmCovCell {
  using Shared = LooMmCovShared;
  static constexpr int kCandidates = 3;
  const LooMmGene& g;
  Shared& ms;
  static int fields(int C) { return loo_mm_cov_fields(C); }
  // ms null: an unmatched cell, the identity and zeros
  static void store(double* o, int C, double elpd, double p_loo, double looic, double khat, double khat_before, int iterations,
                    int cov_iterations, const Shared* ms) {
    loo_mm_cov_store(o, C, elpd, p_loo, looic, khat, khat_before, iterations, cov_iterations, ms ? ms->M : nullptr, ms ? ms->b : nullptr);
  }
  void identity() {
    loo_mm_cov_identity(ms.M, ms.b, g.C + 1);
    loo_mm_cov_identity(ms.Minv, nullptr, g.C + 1);
    ms.logJ = 0.0;
  }
  LooMmAffine state(int cand) const {
    return cand == 0 ? LooMmAffine{ms.M, ms.b} : cand == 1 ? LooMmAffine{ms.M, ms.b1} : cand == 2 ? LooMmAffine{ms.M2, ms.b2}
                                                                                                   : LooMmAffine{ms.M3, ms.b3};
  }
  void keep(int c, bool coord, const LooMmMoments& mo) { if (coord) { ms.m[c] = mo.m; ms.mw[c] = mo.mw; ms.sc[c] = mo.sc; } }
  void form_candidates() { loo_mm_cov_cand12(g, ms.M, ms.b, ms.m, ms.mw, ms.sc, ms.b1, ms.M2, ms.b2); }
  // step 5 before candidate 3: sum w^2, per pair (a <= b) one sweep for the two centred sums, the factorisation and the candidate
  bool prepare(int cand, long n, const double* W, double lse) {
    PPCX_NO_CONTRACT
    if (cand != 3) return true;
    const int nc = g.C + 1, d = loo_mm_cov_dim(g);
    const LooMmAffine cur = state(0);
    double sw2 = 0.0;
    for (long i = 0; i < n; ++i) { const double w = exp(W[i] - lse); sw2 += w * w; }
    for (int ia = 0; ia < d; ++ia)
      for (int ib = ia; ib < d; ++ib) {
        const int ra = loo_mm_cov_row(g, ia), rb = loo_mm_cov_row(g, ib);
        const double ma = ms.m[ra], mb = ms.m[rb], mwa = ms.mw[ra], mwb = ms.mw[rb];
        double sa = 0.0, sw = 0.0;
        for (long i = 0; i < n; ++i) {
          const double ta = cur.coord(g, ra, i), tb = cur.coord(g, rb, i);
          const double w = exp(W[i] - lse);
          sa += (ta - ma) * (tb - mb);
          sw += w * ((ta - mwa) * (tb - mwb));
        }
        ms.SA[ib * nc + ia] = sa; ms.SB[ib * nc + ia] = sw;
      }
    ms.dlogJ = 0.0;
    return loo_mm_cov_cand3(g, sw2, ms.m, ms.mw, ms.SA, ms.SB, ms.M, ms.b, ms.Tm, ms.Tinv, ms.M3, ms.b3, &ms.dlogJ);
  }
  void accept(int cand) {
    const int nc = g.C + 1;
    const LooMmAffine c = state(cand);
    loo_mm_cov_accept_inverse(g, cand, ms.sc, ms.Tinv, ms.dlogJ, ms.Minv, &ms.logJ);
    if (cand != 1) for (int j = 0; j < nc * nc; ++j) ms.M[j] = c.M[j];
    for (int j = 0; j < nc; ++j) ms.b[j] = c.b[j];
  }
};

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <memory>
#include <vector>
namespace ppcx {
// the whole spec for one cell, sequentially, for the CPU check: ppcx_loo_mm.h's cell under the affine state, then step 7:
// out[loo_mm_cov_fields(C)]. kinds (may be null): the accepted candidates in order, 1, 2 or 3. inv (may be null): Minv [nc][nc],
// binv [nc] and logJ of the final state, nc nc + nc + 1 doubles (ppcx_loo_mm_cov_exact.h's loo_mm_cov_inv_fields).
inline void loo_mm_cov_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, bool split, double* out,
                                 std::vector<int>* kinds = nullptr, double* inv = nullptr) {
  PPCX_NO_CONTRACT
  const long n = g.n;
  const int nc = g.C + 1;
  const std::unique_ptr<LooMmCovShared> held(new LooMmCovShared());   // value-initialised: inv's binv of an unmatched cell is zeros
  LooMmCovShared& cs = *held;
  LooMmCovCell cell{g, cs};
  cell.identity();
  double lpd;
  const bool matched = loo_mm_cell_host_as(cell, s, r_eff, k_threshold, max_iters, out, kinds, &lpd);
  if (matched) loo_mm_cov_binv(g, cs.Minv, cs.b, cs.binv);
  if (inv) {
    for (int j = 0; j < nc * nc; ++j) inv[j] = cs.Minv[j];
    for (int c = 0; c < nc; ++c) inv[nc * nc + c] = cs.binv[c];
    inv[nc * nc + nc] = cs.logJ;
  }
  if (!matched || !split) return;
  // ---- step 7: candidate 2's place becomes the identity state, as in the kernel
  loo_mm_cov_identity(cs.M2, cs.b2, nc);
  const long h = loo_mm_split_half(n);
  const LooMmAffine fwd{cs.M, cs.b}, id{cs.M2, cs.b2}, back{cs.Minv, cs.binv};
  std::vector<double> r(n), lx(n), lw, a1, a2;
  bool any = false;
  for (long i = 0; i < n; ++i) {
    r[i] = i < h ? loo_mm_split_ratio(g, i, fwd, id, cs.logJ, s, &lx[i]) : loo_mm_split_ratio(g, i, id, back, cs.logJ, s, &lx[i]);
    any = any || r[i] != -INFINITY;
  }
  const double khat_split = loo_mm_psis_host(r, r_eff, lw);
  if (!any) { loo_mm_cov_store_split_nan(out); return; }
  for (long i = 0; i < n; ++i) if (lw[i] != -INFINITY) { a1.push_back(lw[i] + lx[i]); a2.push_back(lw[i]); }
  loo_mm_cov_store_split(out, loo_logsumexp_host(a1) - loo_logsumexp_host(a2), lpd, khat_split);
}
}  // namespace ppcx
#endif
