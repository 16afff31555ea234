// ppcx_loo_mm_exact.h -- the exact leave-one-out predictive tails and interval of a cell under the moment-matched weights
// (ppcx_fit_loo_predict_exact_moment_match): ppcx_loo_exact.h for the cells that ppcx_loo_mm.h has matched. The cells a
// posterior-predictive check exists to find are outliers, and an outlier is the cell with a high Pareto k: ppcx_fit_loo_predict_exact
// reports that k and its row is not to be trusted; ppcx_fit_loo_moment_match repairs the weights but returns elpd_loo only.
// Its scale and shift are what this header starts from. Restated from Paananen et al. (2021); not run against R.
//
// Shared by the gfx950 kernel (ppcx_loo_mm_exact.hip) and the CPU check (tests/loo_mm_exact_host): the blocks below are
// `__host__ __device__`; loo_mm_exact_cell_host at the end is their sequential composition.
//
// One cell (g, s) from what ppcx_loo_mm.h reads and the record it leaves for the cell (khat, khat_before, iterations, scale A,
// shift B):
//   1. iterations == 0 (a cell that is excluded, NaN, at or below the threshold, run with max_iters = 0, or without an accepted
//      candidate): ppcx_loo_exact.h itself -- the same blocks in the same order, so the ten fields are ppcx_fit_loo_predict_exact's
//      bit for bit (an excluded cell: ppcx_fit_ppc_exact's nine and khat = NaN). The matched path is NOT evaluated at
//      (A, B) = (1, 0) for these cells: q - Q0 - ll equals -ll only up to rounding.
//   2. iterations > 0, the weights. With t_i = A theta_i + B formed from the table, never stored:
//      r_i = loo_mm_ratio(q(t_i; h_i), Q0_i, ll_gs(t_i)), q by loo_mm_density at the state and Q0_i by it at the identity, in the
//      same visit of draw i; PSIS on r as ppcx_loo_mm.h step 3 runs it (the tail length from the participating draws and r_eff,
//      the tie rule, -Inf: the draw takes no part), w_i = exp(lw_i - max lw) / sum as ppcx_loo_exact.h step 1. These are the
//      ratios of the candidate that ppcx_loo_mm.h accepted last, so khat is its final khat bit for bit.
//   3. iterations > 0, the predictive, at the TRANSFORMED draws: eta_i = loo_mm_eta(.., t), sigma_raw_i = t_{C,i},
//      ln phi_i = ppc_exact_lnphi(sigma_raw_i, ln tc), then ppc_exact_sweeps over (w, eta, ln phi) with den = 1. Importance sampling
//      with the transformed draws as the proposal; the Jacobian is the same for every draw and cancels in the normalised
//      weights. A transformed draw with invalid parameters (ppc_exact_invalid) makes the cell's statistics NaN, khat included.
//   4. The fields: the ten of ppcx_loo_exact.h with khat the final one, then khat_before, iterations, scale[C + 1], shift[C + 1]
//      in the table's row order.
//   5. Left out, as in ppcx_loo_mm.h: the split transformation and the covariance step. A matched khat therefore stays
//      necessary, not sufficient; mcse / n_eff of a matched cell are not estimated. The split transformation is
//      ppcx_loo_mm_split.h (ppcx_fit_loo_predict_exact_moment_match_split); the covariance step is ppcx_loo_mm_cov_exact.h
//      (ppcx_fit_loo_predict_exact_moment_match_cov).
// Every sum runs in a fixed order with contraction off: a cell's fields depend on its own gene's data only.
#pragma once
#include <stdint.h>
#include "ppcx_loo_mm.h"
#include "ppcx_loo_exact.h"

namespace ppcx {

constexpr int kLooMmExactHead = kLooExactFields + 2;   // ppcx_loo_exact.h's ten, khat_before, iterations (include/ppcx.h)
PPCX_HD int loo_mm_exact_fields(int C) { return kLooMmExactHead + 2 * (C + 1); }   // PPCX_LOO_MM_EXACT_FIELDS(C)

// step 2: the ratio of draw i under the state (A, B); one / zero: the identity state [C + 1]
PPCX_HD double loo_mm_exact_ratio(const LooMmGene& g, long i, const double* A, const double* B, const double* one, const double* zero,
                                  int s) {
  double l, l0;
  const double q = loo_mm_density(g, i, A, B, s, &l);
  const double q0 = loo_mm_density(g, i, one, zero, s, &l0);
  return loo_mm_ratio(q, q0, l);
}
// step 3: the linear predictor and sigma_raw of the cell of sample s at the transformed draw i
PPCX_HD double loo_mm_exact_eta(const LooMmGene& g, int s, long i, const double* A, const double* B, double* sigma_raw) {
  *sigma_raw = loo_mm_coord(g, g.C, i, A, B);
  return loo_mm_eta(g, s, i, loo_mm_coord(g, 0, i, A, B), A, B);
}
// step 4: the tail of a cell's record behind its ten fields, from the record rec[loo_mm_fields(C)] of ppcx_loo_mm.h
PPCX_HD void loo_mm_exact_store_state(double* o, int C, const double* rec) {
  o[kLooExactFields] = rec[4]; o[kLooExactFields + 1] = rec[5];
  for (int c = 0; c < 2 * (C + 1); ++c) o[kLooMmExactHead + c] = rec[kLooMmHead + c];
}

}  // namespace ppcx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
namespace ppcx {
// step 1: ppcx_loo_exact.h itself on the original draws of the cell, the ten fields into out
inline void loo_mm_exact_unmatched_host(const LooMmGene& g, int s, double r_eff, double tc, double p_lo, double p_hi, double* out) {
  const long n = g.n;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  const std::vector<double> one((size_t)g.C + 1, 1.0), zero((size_t)g.C + 1, 0.0);
  std::vector<double> eta((size_t)n), sg((size_t)n), ll((size_t)n);
  for (long i = 0; i < n; ++i) {
    eta[i] = loo_mm_exact_eta(g, s, i, one.data(), zero.data(), &sg[i]);
    ll[i] = loo_ll(y, eta[i], sg[i]);
  }
  loo_exact_cell_host(ll.data(), eta.data(), sg.data(), nullptr, n, y, excluded, r_eff, tc, p_lo, p_hi, out);
}
// the log weights w[0 .. n) into the normalised weights exp(w - max) / sum (ppcx_loo_exact.h step 1); false, and w untouched,
// where no draw has a log weight above -Inf
inline bool loo_mm_normalise_host(std::vector<double>& w) {
  PPCX_NO_CONTRACT
  double mxw = -INFINITY, sw = 0.0;
  for (double x : w) mxw = x > mxw ? x : mxw;
  if (mxw == -INFINITY) return false;
  for (double& x : w) { x = exp(x - mxw); sw += x; }
  for (double& x : w) x = x / sw;
  return true;
}
// step 3: the predictive under the normalised weights w at the states state(i) -> (A, B) of every draw: the nine fields of
// ppc_exact_sweeps into out and true, or the cell's NaN record and false (an invalid draw, a failed sweep)
template <class F>
inline bool loo_mm_predictive_host(const LooMmGene& g, int s, const std::vector<double>& w, double tc, double p_lo, double p_hi, double* out,
                                   F state) {
  PPCX_NO_CONTRACT
  const long n = g.n;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  const double log_tc = log(tc);
  std::vector<double> eta((size_t)n), sg((size_t)n);
  for (long i = 0; i < n; ++i) {
    const double *A, *B;
    state(i, &A, &B);
    eta[i] = loo_mm_exact_eta(g, s, i, A, B, &sg[i]);
    if (ppc_exact_invalid(eta[i], ppc_exact_phi(ppc_exact_lnphi(sg[i], log_tc)))) { loo_exact_store_nan(out, y, excluded); return false; }
  }
  int mx = 0;
  return ppc_exact_sweeps(ExactHostSums{w.data(), eta.data(), sg.data(), log_tc, n, &mx}, y, excluded, 1, p_lo, p_hi, true, out);
}
// the whole spec for one cell, sequentially, for the CPU check: out[loo_mm_exact_fields(C)]
inline void loo_mm_exact_cell_host(const LooMmGene& g, int s, double r_eff, double k_threshold, int max_iters, double tc, double p_lo,
                                   double p_hi, double* out) {
  const long n = g.n;
  const int C = g.C, nc = C + 1;
  const bool excluded = g.yrow[s] < 0;
  const int y = excluded ? -g.yrow[s] - 1 : g.yrow[s];
  std::vector<double> rec((size_t)loo_mm_fields(C));
  loo_mm_cell_host(g, s, r_eff, k_threshold, max_iters, rec.data());
  loo_mm_exact_store_state(out, C, rec.data());
  if ((int)rec[5] == 0) { loo_mm_exact_unmatched_host(g, s, r_eff, tc, p_lo, p_hi, out); return; }
  // ---- step 2
  const std::vector<double> one((size_t)nc, 1.0), zero((size_t)nc, 0.0);
  const double* A = rec.data() + kLooMmHead;
  const double* B = A + nc;
  std::vector<double> r((size_t)n), w;
  for (long i = 0; i < n; ++i) r[i] = loo_mm_exact_ratio(g, i, A, B, one.data(), zero.data(), s);
  const double khat = loo_mm_psis_host(r, r_eff, w);
  if (!loo_mm_normalise_host(w)) { loo_exact_store_nan(out, y, excluded); return; }
  // ---- step 3
  const bool ok = loo_mm_predictive_host(g, s, w, tc, p_lo, p_hi, out, [&](long, const double** a, const double** b) { *a = A; *b = B; });
  out[kPpcExactFields] = ok ? khat : NAN;
}
}  // namespace ppcx
#endif
