// ppcx_loo_mm.h -- gene-local moment matching for the PSIS-LOO cells with a high Pareto k (ppcx_fit_loo_moment_match): the
// importance-weighted moment matching of Paananen, Piironen, Buerkner, Vehtari (2021), "Implicitly adaptive importance sampling"
// (loo::loo_moment_match), restated for this model and applied to the coordinates of ONE gene. Restated from the paper; not
// run against R.
//
// Why one gene is enough. The importance ratio of cell (g, s) depends on gene g's own coordinates theta_g only: intercept_g,
// sigma_raw_g and, for a checked gene of a design with C >= 2 columns, its C - 1 slopes (d = 2 .. C + 1 <= 17). Given the six
// hyper-parameters the posterior factorises over the genes, so an affine transform of theta_g alone changes the log posterior
// by the gene's own terms: the log-likelihoods of its cells and its prior terms, as gene_close (ppcx_model.h) states them.
// Neither the full log_prob nor lp__ is needed, so a fit over pooled chains (ppcx_fit_from_draws) is served. loo transforms
// all D coordinates; with D in the thousands and a handful of effective draws its weighted moments of the other genes are
// noise, while the leave-one-cell-out posterior differs from the full one in theta_g and barely anywhere else. This is a
// deliberate deviation from loo.
//
// Shared by the gfx950 kernel (ppcx_loo_mm.hip) and the CPU check (tests/loo_mm_host): the blocks below are
// `__host__ __device__`; loo_mm_cell_host at the end is their sequential composition. The local density (the prior, eta, q and
// the cell's log-likelihood), the moment sweeps and the sequential cell are stated here once, over a state's point and a policy:
// ppcx_loo_mm_cov.h instantiates them with its affine state. The two kernels keep a body each over the one density
// (ppcx_loo_mm.hip, ppcx_loo_mm_cov.hip).
//
// One cell (g, s) from the gene's rows of the transposed table T[c][draw] (c = 0 intercept, 1 .. C - 1 slopes, C sigma_raw), the
// draws' six unconstrained hyper-parameters U[k][draw], the gene's encoded counts, r_eff, k_threshold and max_iters:
//   0. ppcx_fit_loo's steps unchanged (ppcx_loo.h). A cell that is excluded, or NaN, or has khat <= k_threshold, or is run with
//      max_iters = 0, is finished: its first four fields are ppcx_fit_loo's bits, khat_before = khat, iterations = 0, every
//      scale 1 and every shift 0. So is a cell on which no candidate of step 3 is accepted.
//   1. The local density q(theta_g; h_i) = sum over the cells s' of the gene that the model does not exclude now of
//      ll(y_gs', eta_s', sigma_raw) + the gene's prior terms: -z^2 / 2 + log erfc(-lambda_skew z / sqrt 2), z = (intercept - xi) /
//      lambda_sigma; -(sigma_raw - (sigma_slope intercept + sigma_intercept))^2 / (2 sigma_sigma^2); for a checked gene -|alpha_1|
//      and -alpha_c^2 / 12.5 (c >= 2). The terms of those priors that do not depend on theta_g are left out. h_i = make_hyper of
//      draw i's hyper-parameters. Q0_i = q(theta_g,i; h_i) at the original draws is kept for the whole cell.
//   2. The state: every coordinate c carries (A_c, B_c), initially (1, 0); the current draws are t_ic = A_c theta_ic + B_c,
//      formed from the table where they are needed, never stored. A row that is no coordinate of the gene (the slopes of a gene
//      that is not checked) keeps (1, 0).
//   3. While k > k_threshold and iterations < max_iters: with w_i the current normalised weights (smoothed and truncated,
//      ppcx_loo.h step 3; the log weight of a draw under the tie rule of ppcx_loo_predict.h) and, per coordinate, over all n draws
//        m = mean t_i,  v = sum (t_i - m)^2 / (n - 1),  mw = sum w_i t_i,  vw = sum w_i t_i^2 - mw^2:
//        candidate 1 (shift):            B' = B + (mw - m);
//        candidate 2 (shift and scale):  s = sqrt(vw / v), A' = s A, B' = s (B - m) + mw; invalid unless every s is finite and > 0.
//      A candidate's ratios are r_i = q(t'_i; h_i) - Q0_i - ll_gs(t'_i); a value that is not finite becomes -Inf (the draw takes
//      no part). The cell's PSIS on r (the tail length by psis_tail_len from the participating draws and the same r_eff) gives
//      k'. The candidate is accepted when k' < k, strictly (a NaN or +Inf k' never passes). Candidate 1 first, candidate 2 only
//      if 1 is refused, as loo does. An accepted candidate becomes the state, its weights the current ones, iterations += 1;
//      if neither is accepted the loop ends. The Jacobian of the transform is the same for every draw and cancels.
//   4. elpd_loo = logsumexp(lw + ll_gs(t)) - logsumexp(lw) under the final state; lpd that of the original draws;
//      p_loo = lpd - elpd_loo, looic = -2 elpd_loo, khat the final k, khat_before that of plain PSIS.
//   5. Left out here: the covariance step (it is ppcx_loo_mm_cov.h, ppcx_fit_loo_moment_match_cov, which runs this header's
//      cell on an affine state and adds the third candidate); the split transformation; mcse / n_eff of a matched cell. Without the split step repeated shifts can overshoot on a very fine posterior sample: khat falls below 0.7 while
//      the error of elpd_loo stays at plain PSIS's size (seen on a 2-D grid posterior of 2500 x 2500 points at n = 4000; not at
//      900 x 900). khat of a matched cell is therefore necessary, not sufficient. The split transformation is
//      ppcx_loo_mm_split.h (ppcx_fit_loo_moment_match_split), which starts from this header's record.
// The fields: elpd_loo, p_loo, looic, khat, khat_before, iterations, then scale[C + 1] and shift[C + 1] in the table's row order.
// Every reduction runs in a fixed order with contraction off: a cell's fields depend on its own gene's data only.
#pragma once
#include <stdint.h>
#include "ppcx_model.h"
#include "ppcx_loo.h"

namespace ppcx {

constexpr int kLooMmHead = 6;                  // elpd_loo, p_loo, looic, khat, khat_before, iterations (include/ppcx.h)
PPCX_HD int loo_mm_fields(int C) { return kLooMmHead + 2 * (C + 1); }   // PPCX_LOO_MM_FIELDS(C)

// What the local density of one gene reads
struct LooMmGene {
  const double* Tg = nullptr;      // [C + 1][n] the gene's rows of the transposed table
  const double* U = nullptr;       // [6][n] the draws' unconstrained hyper-parameters, in hyper_index's order
  long n = 0;
  int C = 1, S = 1;
  bool checked = false;            // the gene has slopes (C >= 2) and their priors
  const int* yrow = nullptr;       // [S] the gene's counts, an excluded cell as -(y + 1)
  const double* expo = nullptr;    // [S] exposure
  const double* X = nullptr;       // [C][S] design, column-major
  double lambda_mu_mu = 0.0;
};

// whether row c of the table is a coordinate of the gene
PPCX_HD bool loo_mm_is_coord(const LooMmGene& g, int c) { return c == 0 || c == g.C || g.checked; }
// coordinate c of draw i under the state
PPCX_HD double loo_mm_coord(const LooMmGene& g, int c, long i, const double* A, const double* B) {
  PPCX_NO_CONTRACT
  return A[c] * g.Tg[(long)c * g.n + i] + B[c];
}
// A state maps draw i of the table to a point t: t(c) is row c of the draw under the state. The local density below reads a
// point and nothing else of a state; the moment sweeps read one coordinate at a time (coord). The diagonal state (A, B) forms a
// coordinate where it is read and keeps no array; the affine state is ppcx_loo_mm_cov.h's LooMmAffine.
struct LooMmDiag {
  const double* A; const double* B;
  struct Point {
    const LooMmGene& g; long i; const double* A; const double* B;
    PPCX_HD double operator()(int c) const { return loo_mm_coord(g, c, i, A, B); }
  };
  PPCX_HD double coord(const LooMmGene& g, int c, long i) const { return loo_mm_coord(g, c, i, A, B); }
  PPCX_HD Point point(const LooMmGene& g, long i) const { return Point{g, i, A, B}; }
};
// loo_ll with the dispersion's point formed by the caller (once per draw)
PPCX_HD double loo_mm_ll(int y, double eta, double sigma_raw, const DispPoint& p) {
  PPCX_NO_CONTRACT
  double F, Dh;
  disp_cell(y, p, &F, &Dh);
  const double yd = (double)y;
  const double lw = loo_log1pexp(eta + sigma_raw);
  return yd * eta - yd - (yd + p.phi) * lw + F - lgamma_int1(yd);
}
// linear predictor of sample s at the point t, t0 = t(0)
template <class Point>
PPCX_HD double loo_mm_eta_at(const LooMmGene& g, int s, double t0, const Point& t) {
  PPCX_NO_CONTRACT
  double eta = g.expo[s] + g.X[s] * t0;
  for (int c = 1; c < g.C; ++c) eta += g.X[(long)c * g.S + s] * t(c);
  return eta;
}
// the gene's prior terms at draw i's hyper-parameters and the point t (step 1), t0 = t(0), sg = t(C)
template <class Point>
PPCX_HD double loo_mm_prior_at(const LooMmGene& g, long i, double t0, double sg, const Point& t) {
  PPCX_NO_CONTRACT
  double u6[6];
  for (int k = 0; k < 6; ++k) u6[k] = g.U[(long)k * g.n + i];
  const Hyper h = make_hyper(u6, g.lambda_mu_mu);
  const double z = (t0 - h.xi) * h.inv_om;
  double lerfc, ratio;
  log_erfc_and_ratio(-h.lambda_skew * z * 0.70710678118654752440, &lerfc, &ratio);
  double lp = -0.5 * z * z + lerfc;
  const double r = sg - (h.sigma_slope * t0 + h.sigma_intercept);
  lp += -0.5 * r * (r * h.inv_ss2);
  if (g.checked) {
    for (int c = 1; c < g.C; ++c) {
      const double al = t(c);
      lp += c == 1 ? -fabs(al) : -(al * al) / 12.5;
    }
  }
  return lp;
}
// q(t_i; h_i) of step 1 under the state, and the log-likelihood of the cell of sample s_cell itself (whether excluded or not)
template <class State>
PPCX_HD double loo_mm_density(const LooMmGene& g, long i, const State& st, int s_cell, double* ll_cell) {
  PPCX_NO_CONTRACT
  const auto t = st.point(g, i);
  const double t0 = t(0), sg = t(g.C);
  const DispPoint p = disp_point(sg);
  double q = 0.0;
  for (int s = 0; s < g.S; ++s) {
    const int ye = g.yrow[s];
    if (ye < 0 && s != s_cell) continue;
    const double ll = loo_mm_ll(ye < 0 ? -ye - 1 : ye, loo_mm_eta_at(g, s, t0, t), sg, p);
    if (ye >= 0) q += ll;
    if (s == s_cell) *ll_cell = ll;
  }
  return q + loo_mm_prior_at(g, i, t0, sg, t);
}
// the log-likelihood of the cell of sample s alone, under the state (step 4)
template <class State>
PPCX_HD double loo_mm_cell_ll(const LooMmGene& g, long i, const State& st, int s) {
  PPCX_NO_CONTRACT
  const auto t = st.point(g, i);
  const double t0 = t(0), sg = t(g.C);
  const int ye = g.yrow[s];
  return loo_mm_ll(ye < 0 ? -ye - 1 : ye, loo_mm_eta_at(g, s, t0, t), sg, disp_point(sg));
}
// the same under the diagonal state given by its arrays (ppcx_loo_mm_exact.h, ppcx_loo_mm_split.h, tests/loo_mm_host)
PPCX_HD double loo_mm_eta(const LooMmGene& g, int s, long i, double t0, const double* A, const double* B) {
  return loo_mm_eta_at(g, s, t0, LooMmDiag{A, B}.point(g, i));
}
PPCX_HD double loo_mm_density(const LooMmGene& g, long i, const double* A, const double* B, int s_cell, double* ll_cell) {
  return loo_mm_density(g, i, LooMmDiag{A, B}, s_cell, ll_cell);
}
PPCX_HD double loo_mm_cell_ll(const LooMmGene& g, long i, const double* A, const double* B, int s) {
  return loo_mm_cell_ll(g, i, LooMmDiag{A, B}, s);
}
// a candidate's ratio at one draw (step 3)
PPCX_HD double loo_mm_ratio(double q, double q0, double ll) {
  PPCX_NO_CONTRACT
  const double r = q - q0 - ll;
  return isfinite(r) ? r : -INFINITY;
}
// the moments of one coordinate from its sums: st = sum t, sd2 = sum (t - m)^2, swt = sum w t, swt2 = sum w t^2
PPCX_HD double loo_mm_mean(double st, long n) { return st / (double)n; }
PPCX_HD double loo_mm_var(double sd2, long n) { return sd2 / (double)(n - 1); }
PPCX_HD double loo_mm_wvar(double swt2, double mw) { PPCX_NO_CONTRACT return swt2 - mw * mw; }
// candidate 1, candidate 2 and its validity
PPCX_HD double loo_mm_shift(double B, double m, double mw) { PPCX_NO_CONTRACT return B + (mw - m); }
PPCX_HD double loo_mm_scale(double vw, double v) { return sqrt(vw / v); }
PPCX_HD bool loo_mm_scale_ok(double s) { return isfinite(s) && s > 0.0; }
PPCX_HD double loo_mm_scaled_A(double s, double A) { return s * A; }
PPCX_HD double loo_mm_scaled_B(double s, double B, double m, double mw) { PPCX_NO_CONTRACT return s * (B - m) + mw; }
// whether a cell is finished after plain PSIS (step 0)
PPCX_HD bool loo_mm_finished(bool excluded, double khat, double k_threshold, int max_iters) {
  return excluded || max_iters <= 0 || !(khat > k_threshold);
}
// the tail of a cell's record behind its first four fields: khat_before, iterations, scale[C + 1], shift[C + 1]
PPCX_HD void loo_mm_store_state(double* o, int C, double khat_before, int iterations, const double* A, const double* B) {
  o[4] = khat_before; o[5] = (double)iterations;
  for (int c = 0; c <= C; ++c) { o[kLooMmHead + c] = A ? A[c] : 1.0; o[kLooMmHead + C + 1 + c] = B ? B[c] : 0.0; }
}

// ---- what the sequential cells of both states share beside the density.
// Step 3's moments of coordinate c under the state `cur` and the weights exp(W[i] - lse), two sweeps over the draws: m, mw and
// the scale sc = sqrt(vw / v). The kernels state the same two sweeps over their workgroup (ppcx_loo_mm.hip, ppcx_loo_mm_cov.hip).
struct LooMmMoments { double m, mw, sc; };
template <class State>
inline LooMmMoments loo_mm_coord_moments(const LooMmGene& g, const State& cur, int c, long n, const double* W, double lse) {
  PPCX_NO_CONTRACT
  double st = 0.0, swt = 0.0, swt2 = 0.0, sd2 = 0.0;
  for (long i = 0; i < n; ++i) {
    const double t = cur.coord(g, c, i), w = exp(W[i] - lse);
    st += t; swt += w * t; swt2 += w * (t * t);
  }
  const double m = loo_mm_mean(st, n);
  for (long i = 0; i < n; ++i) { const double d = cur.coord(g, c, i) - m; sd2 += d * d; }
  const double v = loo_mm_var(sd2, n), vw = loo_mm_wvar(swt2, swt);
  return LooMmMoments{m, swt, loo_mm_scale(vw, v)};
}

// The sequential cell (loo_mm_cell_host_as below) runs under a policy that owns what differs between the states: the record
// (fields, store), the identity, the state and candidate 1 .. kCandidates as a point's source (state(cand), 0 the current one),
// what is kept of a coordinate's moments (keep; coord false: a row that is no coordinate keeps its state in every candidate) and
// how the candidates are formed from them (form_candidates), what a candidate needs before its density sweep (prepare: false
// refuses it and ends the iteration) and what an accepted step does (accept). LooMmDiagCell is the per-coordinate state of this
// header, ppcx_loo_mm_cov.h's LooMmCovCell the affine one.
// ok2: unused; keeps the static LDS of ppcx_loo_mm_kernel at 3 712 bytes
struct LooMmShared { double A[kMaxC + 1], B[kMaxC + 1], A1[kMaxC + 1], B1[kMaxC + 1], A2[kMaxC + 1], B2[kMaxC + 1]; int ok2; };
struct LooMmDiagCell {
  using Shared = LooMmShared;
  static constexpr int kCandidates = 2;
  const LooMmGene& g;
  Shared& ms;
  static int fields(int C) { return loo_mm_fields(C); }
  // ms null: an unmatched cell, scales 1 and shifts 0
  static void store(double* o, int C, double elpd, double p_loo, double looic, double khat, double khat_before, int iterations, int,
                    const Shared* ms) {
    o[0] = elpd; o[1] = p_loo; o[2] = looic; o[3] = khat;
    loo_mm_store_state(o, C, khat_before, iterations, ms ? ms->A : nullptr, ms ? ms->B : nullptr);
  }
  void identity() { for (int c = 0; c <= g.C; ++c) { ms.A[c] = 1.0; ms.B[c] = 0.0; } }
  LooMmDiag state(int cand) const {
    return cand == 0 ? LooMmDiag{ms.A, ms.B} : cand == 1 ? LooMmDiag{ms.A1, ms.B1} : LooMmDiag{ms.A2, ms.B2};
  }
  void keep(int c, bool coord, const LooMmMoments& mo) {
    ms.A1[c] = ms.A[c]; ms.B1[c] = coord ? loo_mm_shift(ms.B[c], mo.m, mo.mw) : ms.B[c];
    ms.A2[c] = coord ? loo_mm_scaled_A(mo.sc, ms.A[c]) : ms.A[c];
    ms.B2[c] = coord ? loo_mm_scaled_B(mo.sc, ms.B[c], mo.m, mo.mw) : ms.B[c];
  }
  void form_candidates() {}
  bool prepare(int, long, const double*, double) { return true; }
  void accept(int cand) {
    const LooMmDiag c = state(cand);
    for (int j = 0; j <= g.C; ++j) { ms.A[j] = c.A[j]; ms.B[j] = c.B[j]; }
  }
};

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#include "ppcx_loo_exact.h"
namespace ppcx {
// PSIS of a candidate's ratios r[0 .. n) (-Inf: no part): the log weight of every draw in draw order and k-hat; +Inf without a
// participating draw
inline double loo_mm_psis_host(const std::vector<double>& r, double r_eff, std::vector<double>& lw) {
  bool any = false;
  for (double x : r) any = any || x != -INFINITY;
  if (!any) { lw.assign(r.size(), -INFINITY); return INFINITY; }
  double khat;
  loo_exact_log_weights_host(r.data(), (long)r.size(), r_eff, lw, &khat);
  return khat;
}
// lpd of the original draws from the cell's log-likelihoods ll[0 .. n): log mean exp over the draws that take part (-ll is not
// -Inf); false, and *lpd NaN, without one
inline bool loo_mm_lpd_host(const std::vector<double>& ll, double* lpd) {
  std::vector<double> part;
  for (double l : ll) if (-l != -INFINITY) part.push_back(l);
  *lpd = part.empty() ? NAN : loo_logsumexp_host(part) - log((double)part.size());
  return !part.empty();
}
// The whole spec for one cell, sequentially, for the CPU checks, under the policy `cell` at its identity: out[Cell::fields(C)].
// kinds (may be null): the accepted candidates in order. Returns whether the cell was matched (iterations > 0); then *lpd is
// that of the original draws and the final state is cell.ms's.
template <class Cell>
inline bool loo_mm_cell_host_as(Cell& cell, int s, double r_eff, double k_threshold, int max_iters, double* out, std::vector<int>* kinds,
                                double* lpd) {
  PPCX_NO_CONTRACT
  const LooMmGene& g = cell.g;
  const long n = g.n;
  const int C = g.C;
  const bool excluded = g.yrow[s] < 0;
  if (kinds) kinds->clear();
  // ---- step 0
  std::vector<double> ll(n);
  for (long i = 0; i < n; ++i) ll[i] = loo_mm_cell_ll(g, i, cell.state(0), s);
  double loo4[kLooFields];
  loo_cell_host(ll.data(), n, r_eff, excluded, loo4);
  Cell::store(out, C, loo4[0], loo4[1], loo4[2], loo4[3], loo4[3], 0, 0, nullptr);
  if (loo_mm_finished(excluded, loo4[3], k_threshold, max_iters)) return false;
  std::vector<double> r(n), lw, lw2;
  for (long i = 0; i < n; ++i) r[i] = -ll[i];
  if (!loo_mm_lpd_host(ll, lpd)) return false;
  double k = loo_mm_psis_host(r, r_eff, lw);
  // ---- step 1 at the original draws
  std::vector<double> Q0(n);
  for (long i = 0; i < n; ++i) { double l; Q0[i] = loo_mm_density(g, i, cell.state(0), s, &l); }
  // ---- step 3
  int iters = 0, cov_iters = 0;
  while (k > k_threshold && iters < max_iters) {
    const double lse = loo_logsumexp_host(lw);
    bool ok2 = true;
    for (int c = 0; c <= C; ++c) {
      const bool coord = loo_mm_is_coord(g, c);
      LooMmMoments mo{0.0, 0.0, 1.0};
      if (coord) { mo = loo_mm_coord_moments(g, cell.state(0), c, n, lw.data(), lse); ok2 = ok2 && loo_mm_scale_ok(mo.sc); }
      cell.keep(c, coord, mo);
    }
    cell.form_candidates();
    int kind = 0;
    for (int cand = 1; cand <= Cell::kCandidates && !kind; ++cand) {
      if (cand == 2 && !ok2) continue;
      if (!cell.prepare(cand, n, lw.data(), lse)) break;
      const auto st = cell.state(cand);
      for (long i = 0; i < n; ++i) { double l; const double q = loo_mm_density(g, i, st, s, &l); r[i] = loo_mm_ratio(q, Q0[i], l); }
      const double k2 = loo_mm_psis_host(r, r_eff, lw2);
      if (k2 < k) { kind = cand; k = k2; lw = lw2; cell.accept(cand); }
    }
    if (!kind) break;
    ++iters;
    cov_iters += kind == 3;
    if (kinds) kinds->push_back(kind);
  }
  if (iters == 0) return false;
  // ---- step 4
  std::vector<double> a, b;
  for (long i = 0; i < n; ++i)
    if (lw[i] != -INFINITY) { a.push_back(lw[i] + loo_mm_cell_ll(g, i, cell.state(0), s)); b.push_back(lw[i]); }
  const double elpd = loo_logsumexp_host(a) - loo_logsumexp_host(b);
  Cell::store(out, C, elpd, *lpd - elpd, -2.0 * elpd, k, loo4[3], iters, cov_iters, &cell.ms);
  return true;
}
// the per-coordinate state's: out[loo_mm_fields(C)], kinds 1 or 2
inline void loo_mm_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, double* out,
                             std::vector<int>* kinds = nullptr) {
  LooMmShared ms;
  LooMmDiagCell cell{g, ms};
  cell.identity();
  double lpd;
  loo_mm_cell_host_as(cell, s, r_eff, k_threshold, max_iters, out, kinds, &lpd);
}
}  // namespace ppcx
#endif
