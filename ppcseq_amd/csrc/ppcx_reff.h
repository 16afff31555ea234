// ppcx_reff.h -- the relative efficiency of the importance ratios per observed cell of a NUTS fit (ppcx_fit_relative_eff): what
// rstan::loo(fit) passes to loo::loo as r_eff, loo::relative_eff(exp(log_lik), chain_id). The draws of a NUTS fit are
// autocorrelated, and the PSIS tail length depends on it: M = ceil(min(0.2 N, 3 sqrt(N / r_eff))) (ppcx_loo.h step 1).
//
// Shared by the gfx950 kernel (ppcx_reff.hip, one workgroup per cell) and the CPU check (tests/reff_host): relative_eff_cell_host
// below is the sequential composition of ppcx_summary.h's blocks, the kernel composes the same blocks with workgroup-parallel
// loops (ppcx_summary_dev.h).
//
// Spec of one cell with the log-likelihoods ll[c][i] of a fit with M chains of n kept draws (chain-major, ll[c * n + i]):
//   split chains as ppcx_summary.h does: n' = floor(n / 2), chain c gives sequences 2c (its first n' draws) and 2c + 1 (its last
//   n'; an odd n drops the middle draw), m = 2M sequences, N = m n' split values (split_source);
//   v = exp(ll - L), L the largest ll among the split values. The ESS does not depend on the scale of v, so this is
//   relative_eff(exp(log_lik)) wherever exp(ll) does not underflow, and stays defined where it does;
//   ESS = the Geyer estimator of the fit summary (var_plus_of, rho_of, Geyer, floor 1 / log10(N)) on v itself over the m
//   sequences -- no rank normalisation, no folding: posterior::ess_mean, which loo::relative_eff calls for draws by chains;
//   r_eff = ESS / N. Values above 1 (antithetic chains) are kept as they are.
//   NaN: a NaN or +Inf ll among the split values; n' < 2; all split values equal (var_plus not > 0).
//   ll = -Inf gives v = 0 and is an ordinary value.
// An excluded cell gets a value like any other (its log-likelihood is defined); ppcx_fit_loo never uses it.
// Every reduction runs in a fixed order: a cell's value depends on its own column only.
#pragma once
#include "ppcx_summary.h"

namespace ppcx {

#if !defined(__HIP_DEVICE_COMPILE__)
// the whole spec for one cell, sequentially, for the CPU check; work: m n' doubles
inline double relative_eff_cell_host(const double* ll, int M, int n) {
  const int nh = n / 2, m = 2 * M;
  const long N = (long)m * nh;
  if (nh < 2 || M < 1) return NAN;
  double* z = new double[N];
  double L = -INFINITY; bool bad = false;
  for (long k = 0; k < N; ++k) {
    const double v = ll[split_source(k, nh, n)];
    bad = bad || isnan(v) || v == INFINITY;
    L = v > L ? v : L;
    z[k] = v;
  }
  double ess = NAN;
  if (!bad && L != -INFINITY) {                 // all -Inf: every value equal
    for (long k = 0; k < N; ++k) z[k] = exp(z[k] - L);
    summary_seq_host(z, m, nh, &ess);
  }
  delete[] z;
  return ess / (double)N;
}
#endif

}  // namespace ppcx
