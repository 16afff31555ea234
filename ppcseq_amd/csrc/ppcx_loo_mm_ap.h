// ppcx_loo_mm_ap.h -- gene-local moment matching for the PSIS-LOO cells of an ADVI fit with a high Pareto k
// (ppcx_fit_loo_moment_match_approx) and the exact leave-one-out predictive under its weights
// (ppcx_fit_loo_predict_exact_moment_match_approx): ppcx_loo_mm.h and ppcx_loo_mm_exact.h for draws that come from the
// approximation g, not from the posterior p. loo::loo_moment_match has no approximate-posterior form: this is a deliberate
// deviation from loo, restated from Paananen, Piironen, Buerkner, Vehtari (2021), "Implicitly adaptive importance sampling", and
// Magnusson, Andersen, Jonasson, Vehtari (2019), "Bayesian leave-one-out cross-validation for large data"; not run against R.
//
// Why the gene-local construction carries over. The draws theta_i come from g and the target is the posterior without cell
// (g, s), so the importance ratio of a draw is p(theta) / (g(theta) lik_gs(theta)) (ppcx_loo_ap.h). An affine map T of gene g's
// own coordinates is an implicit change of proposal: the new points are T theta_i and their proposal density is
// g(theta_i) / |det T| -- the same g(theta_i) as before and a constant Jacobian. Given the draw's hyper-parameters the posterior
// factorises over the genes, so log p(T theta_i) - log p(theta_i) is the difference of gene g's local density q(.; h_i) of
// ppcx_loo_mm.h step 1. The log ratio of a candidate state is therefore
//     r_i = a_i + q(t'_i; h_i) - Q0_i - ll_gs(t'_i),     a_i = log_p_i - log_g_i,
// ppcx_loo_mm.h's ratio plus the cached array that ppcx_fit_psis and ppcx_fit_loo_approx run on. The Jacobian is the same for every
// draw and cancels in the normalised weights. Neither log_g at a new point nor (mu, omega) is needed.
//
// Shared by the gfx950 kernels (ppcx_loo_mm.hip and ppcx_loo_mm_exact.hip, their approximate-posterior instantiations) and the
// CPU check (tests/loo_mm_ap_cpu): the blocks below are `__host__ __device__`; loo_mm_ap_cell_host and
// loo_mm_ap_exact_cell_host at the end are their sequential compositions.
//
// One cell (g, s) from what ppcx_loo_mm.h reads and the fit's log ratios a[0 .. n) (-Inf where log_p or log_g is not finite).
// r_eff is 1: an approximation's draws are independent.
//   0. ppcx_loo_ap.h's steps unchanged. A cell that is excluded (its ratios are a_i alone and its khat is the overall k-hat of
//      a), or NaN, or has khat <= k_threshold, or is run with max_iters = 0, is finished: its first four fields are
//      ppcx_fit_loo_approx's bits, khat_before = khat, iterations = 0, every scale 1 and every shift 0. So is a cell on which no
//      candidate of step 2 is accepted.
//   1. Q0_i = q(theta_g,i; h_i) by loo_mm_density at the identity, kept for the whole cell as Qa_i = Q0_i - a_i: ONE rounded
//      subtraction when Q0 is formed (loo_mm_ap_qa). a_i = -Inf makes Qa_i = +Inf and every ratio of the draw -Inf.
//   2. The state, the four moments per coordinate, the two candidates (shift; shift and scale) and the acceptance rule are
//      ppcx_loo_mm.h step 3: k' < k, strictly, the shift tried first. The plain moments m, v are over all n draws, which are
//      draws of the proposal; the weighted ones are under the current normalised weights.
//   3. A candidate's ratios are r_i = loo_mm_ratio(q(t'_i; h_i), Qa_i, ll_gs(t'_i)) = (q - Qa_i) - ll in this order; a value
//      that is not finite becomes -Inf and the draw takes no part. PSIS on r is ppcx_loo_ap.h's steps 1 - 3: the tail length from
//      the participating draws, the tie rule, the smoothing.
//   4. elpd_loo = logsumexp(lw + ll_gs(t)) - logsumexp(lw) under the final state; lpd that of ppcx_loo_ap.h step 4 on the
//      original draws; p_loo = lpd - elpd_loo, looic = -2 elpd_loo, khat the final k, khat_before that of plain PSIS. The
//      fields are loo_mm_fields(C), the layout of ppcx_loo_mm.h.
//   5. The exact predictive under these weights (loo_mm_exact_fields(C), the layout of ppcx_loo_mm_exact.h):
//      iterations == 0: ppcx_loo_exact.h with the log ratios, the ten fields of ppcx_fit_loo_predict_exact_approx bit for bit.
//      iterations > 0: r_i = loo_mm_ratio(q(t_i; h_i), Q0_i - a_i, ll_gs(t_i)) with q and Q0_i formed in the same visit of draw
//      i -- the ratios of the candidate that step 2 accepted last, so khat is its final khat bit for bit --, the normalised
//      weights, and the negative binomials at the transformed draws as ppcx_loo_mm_exact.h steps 2 - 4.
//   6. Left out: the split transformation (for a proposal g it needs log g at inverse-mapped points, hence (mu, omega): a
//      separate statistic); the covariance step; mcse / n_eff; passes over several ranks. Two consequences:
//      - a matched khat below the threshold stays necessary, not sufficient: without the split step a shift can overshoot
//        (one seed of six of the truth case of tests/loo_mm_ap_cases.py gets worse);
//      - the matching moves one gene's coordinates only. If the overall k-hat of a (khat_approximation) is itself above the
//        threshold the mismatch sits in the hyper-parameters as well, and no map of a gene's coordinates repairs that part. A
//        cell's khat is an estimate on the cell's own ratios and can come out below the overall one (a designed cell of
//        tests/loo_mm_ap_cases.py goes from 0.58 to 0.44 under an overall k-hat of 0.62): it does not speak for the
//        hyper-parameters.
// With a all zero a matched cell's record is ppcx_loo_mm.h's at r_eff = 1 bit for bit (0 - ll = -ll and Q0 - 0 = Q0 are exact);
// an unmatched cell's is ppcx_loo_ap.h's, which sums in another order than ppcx_loo.h.
// Every reduction runs in a fixed order with contraction off: a cell's fields depend on its own gene's data and on a only.
#pragma once
#include <stdint.h>
#include "ppcx_loo_mm.h"
#include "ppcx_loo_mm_exact.h"

namespace ppcx {

// step 1: what is kept of Q0_i
PPCX_HD double loo_mm_ap_qa(double q0, double a) {
  PPCX_NO_CONTRACT
  return q0 - a;
}
// step 5: the ratio of draw i under the state (A, B), a = a_i; one / zero: the identity state [C + 1]
PPCX_HD double loo_mm_ap_exact_ratio(const LooMmGene& g, double a, long i, const double* A, const double* B, const double* one,
                                     const double* zero, int s) {
  double l, l0;
  const double q = loo_mm_density(g, i, A, B, s, &l);
  const double q0 = loo_mm_density(g, i, one, zero, s, &l0);
  return loo_mm_ratio(q, loo_mm_ap_qa(q0, a), l);
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
namespace ppcx {
// The whole spec of steps 0 - 4 for one cell, sequentially, for the CPU check: out[loo_mm_fields(C)]. kinds (may be null): the
// accepted candidates in order, 1 or 2.
inline void loo_mm_ap_cell_host(const LooMmGene& g, const double* a, int s, double k_threshold, int max_iters, double* out,
                                std::vector<int>* kinds = nullptr) {
  PPCX_NO_CONTRACT
  const long n = g.n;
  const int C = g.C;
  const bool excluded = g.yrow[s] < 0;
  LooMmShared ms;
  LooMmDiagCell cell{g, ms};
  cell.identity();
  if (kinds) kinds->clear();
  // ---- step 0
  std::vector<double> ll((size_t)n);
  for (long i = 0; i < n; ++i) ll[i] = loo_mm_cell_ll(g, i, cell.state(0), s);
  double loo4[kLooFields];
  loo_ap_cell_host(ll.data(), a, n, excluded, loo4);
  LooMmDiagCell::store(out, C, loo4[0], loo4[1], loo4[2], loo4[3], loo4[3], 0, 0, nullptr);
  if (loo_mm_finished(excluded, loo4[3], k_threshold, max_iters)) return;
  std::vector<double> r, lw, lw2;
  double k;
  if (!loo_ap_weights_host(ll.data(), a, n, false, r, lw, &k)) return;
  std::vector<double> part;
  for (long i = 0; i < n; ++i) if (r[i] != -INFINITY) part.push_back(ll[i]);
  const double lpd = loo_logsumexp_host(part) - log((double)part.size());
  // ---- step 1
  std::vector<double> Qa((size_t)n);
  for (long i = 0; i < n; ++i) { double l; Qa[i] = loo_mm_ap_qa(loo_mm_density(g, i, cell.state(0), s, &l), a[i]); }
  // ---- steps 2 and 3
  int iters = 0;
  while (k > k_threshold && iters < max_iters) {
    const double lse = loo_logsumexp_host(lw);
    bool ok2 = true;
    for (int c = 0; c <= C; ++c) {
      const bool coord = loo_mm_is_coord(g, c);
      LooMmMoments mo{0.0, 0.0, 1.0};
      if (coord) { mo = loo_mm_coord_moments(g, cell.state(0), c, n, lw.data(), lse); ok2 = ok2 && loo_mm_scale_ok(mo.sc); }
      cell.keep(c, coord, mo);
    }
    int kind = 0;
    for (int cand = 1; cand <= LooMmDiagCell::kCandidates && !kind; ++cand) {
      if (cand == 2 && !ok2) continue;
      const LooMmDiag st = cell.state(cand);
      for (long i = 0; i < n; ++i) { double l; const double q = loo_mm_density(g, i, st, s, &l); r[i] = loo_mm_ratio(q, Qa[i], l); }
      const double k2 = loo_mm_psis_host(r, 1.0, lw2);
      if (k2 < k) { kind = cand; k = k2; lw = lw2; cell.accept(cand); }
    }
    if (!kind) break;
    ++iters;
    if (kinds) kinds->push_back(kind);
  }
  if (iters == 0) return;
  // ---- step 4
  std::vector<double> wa, wb;
  for (long i = 0; i < n; ++i)
    if (lw[i] != -INFINITY) { wa.push_back(lw[i] + loo_mm_cell_ll(g, i, cell.state(0), s)); wb.push_back(lw[i]); }
  const double elpd = loo_logsumexp_host(wa) - loo_logsumexp_host(wb);
  LooMmDiagCell::store(out, C, elpd, lpd - elpd, -2.0 * elpd, k, loo4[3], iters, 0, &ms);
}
// The whole spec of step 5 for one cell, sequentially, for the CPU check: out[loo_mm_exact_fields(C)]
inline void loo_mm_ap_exact_cell_host(const LooMmGene& g, const double* a, int s, double k_threshold, int max_iters, double tc, double p_lo,
                                      double p_hi, double* out) {
  const long n = g.n;
  const int C = g.C, nc = C + 1;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  std::vector<double> rec((size_t)loo_mm_fields(C));
  loo_mm_ap_cell_host(g, a, s, k_threshold, max_iters, rec.data());
  loo_mm_exact_store_state(out, C, rec.data());
  const std::vector<double> one((size_t)nc, 1.0), zero((size_t)nc, 0.0);
  if ((int)rec[5] == 0) {                                // ppcx_loo_exact.h itself on the original draws, with the log ratios
    std::vector<double> eta((size_t)n), sg((size_t)n), ll((size_t)n);
    for (long i = 0; i < n; ++i) {
      eta[i] = loo_mm_exact_eta(g, s, i, one.data(), zero.data(), &sg[i]);
      ll[i] = loo_ll(y, eta[i], sg[i]);
    }
    loo_exact_cell_host(ll.data(), eta.data(), sg.data(), a, n, y, excluded, 1.0, tc, p_lo, p_hi, out);
    return;
  }
  const double* A = rec.data() + kLooMmHead;
  const double* B = A + nc;
  std::vector<double> r((size_t)n), w;
  for (long i = 0; i < n; ++i) r[i] = loo_mm_ap_exact_ratio(g, a[i], i, A, B, one.data(), zero.data(), s);
  const double khat = loo_mm_psis_host(r, 1.0, w);
  if (!loo_mm_normalise_host(w)) { loo_exact_store_nan(out, y, excluded); return; }
  const bool ok = loo_mm_predictive_host(g, s, w, tc, p_lo, p_hi, out, [&](long, const double** sa, const double** sb) { *sa = A; *sb = B; });
  out[kPpcExactFields] = ok ? khat : NAN;
}
}  // namespace ppcx
#endif
