// CPU build of the exact leave-one-out predictive under moment-matched weights (ppcseq_amd/csrc/ppcx_loo_mm_exact.h) for
// tests/test_loo_mm_exact_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With
// -DPPCX_HOST_MAIN it is a stand-alone program (a fixed gene, for a run under -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_mm_exact.h"

#define LOO_MM_EXACT_EXPORT extern "C" __attribute__((visibility("default")))

static ppcx::LooMmGene gene_of(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow, const double* expo,
                               const double* X, double lambda_mu_mu) {
  ppcx::LooMmGene g;
  g.Tg = T; g.U = U; g.n = n; g.C = C; g.S = S; g.checked = checked != 0; g.yrow = yrow; g.expo = expo; g.X = X;
  g.lambda_mu_mu = lambda_mu_mu;
  return g;
}

// one cell: T [C + 1][n], U [6][n], yrow [S] (an excluded cell as -(y + 1)), expo [S], X [C][S]; out [12 + 2 (C + 1)]
LOO_MM_EXACT_EXPORT void loo_mm_exact_host_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                                const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff,
                                                double k_threshold, int max_iters, double tc, double p_lo, double p_hi, double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_exact_cell_host(g, s, r_eff, k_threshold, max_iters, tc, p_lo, p_hi, out);
}
// the cell's linear predictor, sigma_raw and log-likelihood [n] at the original draws, as the header forms them for a cell
// that is not matched: what loo_exact_cell_host (tests/loo_exact_host) takes
LOO_MM_EXACT_EXPORT void loo_mm_exact_host_columns(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                                   const double* expo, const double* X, double lambda_mu_mu, int s, double* eta,
                                                   double* sigma_raw, double* ll) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  const std::vector<double> one((size_t)C + 1, 1.0), zero((size_t)C + 1, 0.0);
  const int y = yrow[s] < 0 ? -yrow[s] - 1 : yrow[s];
  for (long i = 0; i < n; ++i) {
    eta[i] = ppcx::loo_mm_exact_eta(g, s, i, one.data(), zero.data(), &sigma_raw[i]);
    ll[i] = ppcx::loo_ll(y, eta[i], sigma_raw[i]);
  }
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
int main() {
  const int C = 2, S = 5;
  const int yrow[S] = {120, 180, -96, 160, 900};
  const double expo[S] = {0.0, 0.1, -0.1, 0.05, 0.0}, X[C * S] = {1, 1, 1, 1, 1, 0, 1, 0, 1, 0};
  int matched = 0;
  for (long n : {1L, 20L, 400L}) {
    std::vector<double> T((C + 1) * n), U(6 * n);
    for (long i = 0; i < n; ++i) {
      T[i] = 5.0 + 0.2 * sin((double)i); T[n + i] = 0.1 * cos(2.0 * (double)i); T[2 * n + i] = -1.0 + 0.3 * sin(5.0 * (double)i);
      const double u[6] = {0.5, 0.6, -1.0, -1.2, 0.0, -0.9};
      for (int k = 0; k < 6; ++k) U[k * n + i] = u[k] + 0.01 * sin((double)(i + k));
    }
    for (int checked = 0; checked < 2; ++checked)
      for (int s : {1, 2, 4}) {
        const ppcx::LooMmGene g = gene_of(T.data(), U.data(), n, C, S, checked, yrow, expo, X, 5.6);
        double out[12 + 2 * (C + 1)];
        ppcx::loo_mm_exact_cell_host(g, s, 0.8, 0.3, 5, 0.7352941, 0.025, 0.975, out);
        printf("n=%ld checked=%d s=%d mean=%.6f sd=%.6f p_le=%.6g p_ge=%.6g lower=%g upper=%g khat=%g before=%g iterations=%g scale=%g %g %g "
               "shift=%g %g %g\n", n, checked, s, out[0], out[1], out[2], out[3], out[4], out[5], out[9], out[10], out[11], out[12], out[13],
               out[14], out[15], out[16], out[17]);
        matched += out[11] > 0.0;
        if (out[4] > out[5]) return 1;
      }
  }
  printf("matched cells: %d\n", matched);
  return matched > 0 ? 0 : 1;
}
#endif
