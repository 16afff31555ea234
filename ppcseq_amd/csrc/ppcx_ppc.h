// ppcx_ppc.h -- the posterior-predictive statistic of a cell (ppcx_fit_ppc, include/ppcx.h), stated once:
// which draw a predictive count comes from, on which Philox address, with which phi, what an impossible draw is recorded as, and
// the type-7 quantiles of the counts. Shared by the gfx950 kernels (ppcx_ppc.hip; the excluded cells of ppcx_loo_predict.hip,
// which must give ppcx_fit_ppc's bits) and the CPU check (ppcx_loo_predict.h, tests/loo_predict_host): everything below is
// `__host__ __device__`.
//
// Cell (g, s) has the Philox address g S + s; its predictive draw j is neg_binomial_2_log_rng(eta, phi) (nb2_log_rng, ppcx_math.h)
// on (seed, address, j), with eta = exposure_s + sum_c X_sc T_c and phi = exp(-sigma_raw) truncation_compensation of posterior
// draw j -- or, resampling, of the posterior draw ppc_resample_src picks. The summary of the n counts is their mean, their sd
// (n - 1) and the type-7 quantiles at p_lo and p_hi from the order statistics around (n - 1) p (select_pair).
#pragma once
#include <stdint.h>
#include "ppcx_math.h"

#ifndef PPCX_NO_CONTRACT
#if defined(__clang__)
#define PPCX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PPCX_NO_CONTRACT
#endif
#endif

namespace ppcx {

constexpr int32_t kPpcInvalid = 2147483647;      // a draw with invalid parameters (nb2_invalid): sorts last
constexpr int32_t kPpcSaturated = 1073741823;    // a Poisson mean of 2^30 or more: Stan raises, we saturate

// the Philox address of cell (gene g of the model, sample s)
PPCX_HD uint32_t ppc_cell_address(int g, int S, int s) { return (uint32_t)(g * S + s); }
// phi of a predictive draw: sigma = 1 ./ exp(sigma_raw), .stan:203,:264
PPCX_HD double ppc_phi(double sigma_raw, double truncation_compensation) {
  PPCX_NO_CONTRACT
  return exp(-sigma_raw) * truncation_compensation;
}
// the posterior draw behind predictive draw j of a resampled cell (R/utilities.R:760: sample(draws, n, replace = TRUE))
PPCX_HD long ppc_resample_src(uint32_t j, uint32_t address, uint32_t k0, long n_draws) {
  const double u = coord_uniform(j, address, 5u, 0u, k0, 0x50504331u);
  const long src = (long)(u * (double)n_draws);
  return src >= n_draws ? n_draws - 1 : src;
}

// type-7 quantile of n values (R quantile default; rstan::summary): h = (n - 1) p rounded on its own -- the product is never
// fused into h - lo --, lo = floor(h) clamped to 0 .. n - 1; from the order statistics v0 (rank lo) and v1 (rank lo + 1) with one
// fma, one rounding as in the oracle
PPCX_HD void type7_rank(long n, double p, double* h_out, long* lo_out) {
  PPCX_NO_CONTRACT
  const double h = (double)(n - 1) * p;
  long lo = (long)floor(h);
  if (lo > n - 1) lo = n - 1;
  if (lo < 0) lo = 0;
  *h_out = h; *lo_out = lo;
}
PPCX_HD double type7(double h, long lo, long n, double v0, double v1) {
  PPCX_NO_CONTRACT
  return lo >= n - 1 ? v0 : fma(h - (double)lo, v1 - v0, v0);
}

// Order statistics r and r + 1 (0-based; the same when r = n - 1) of n integers in 0 .. vmax by bisection on the value: the
// smallest v with #{x <= v} >= r + 1 -- exact, ~log2(vmax) counting passes instead of a sort. count_le(v) = #{x <= v} and
// min_above(v) = the smallest x > v are the caller's: a wavefront's, a workgroup's, a plain loop.
template <class I, class CountLe, class MinAbove>
PPCX_HD void select_pair(I n, I r, int vmax, CountLe count_le, MinAbove min_above, int* v_r, int* v_r1) {
  int lo = 0, hi = vmax;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (count_le(mid) >= r + 1) hi = mid; else lo = mid + 1;
  }
  *v_r = lo;
  // the next order statistic: the same value if it occurs again at rank r + 1, else the smallest value above it
  *v_r1 = r + 1 < n && count_le(lo) < r + 2 ? min_above(lo) : lo;
}

}  // namespace ppcx
