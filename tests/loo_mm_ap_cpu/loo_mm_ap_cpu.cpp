// CPU build of the gene-local moment matching of the PSIS-LOO cells of an ADVI fit and of the exact predictive under its weights
// (ppcseq_amd/csrc/ppcx_loo_mm_ap.h) for tests/test_loo_mm_ap_host.py: the same header the gfx950 kernels include, compiled with
// g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (a fixed gene, for a run under
// -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_mm_ap.h"

#define LOO_MM_AP_EXPORT extern "C" __attribute__((visibility("default")))

static ppcx::LooMmGene gene_of(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow, const double* expo,
                               const double* X, double lambda_mu_mu) {
  ppcx::LooMmGene g;
  g.Tg = T; g.U = U; g.n = n; g.C = C; g.S = S; g.checked = checked != 0; g.yrow = yrow; g.expo = expo; g.X = X;
  g.lambda_mu_mu = lambda_mu_mu;
  return g;
}

// one cell: T [C + 1][n], U [6][n], yrow [S] (an excluded cell as -(y + 1)), expo [S], X [C][S], a [n] the draws' log ratios;
// out [6 + 2 (C + 1)]; kinds [max_iters] receives the accepted candidates (1 or 2) in order. Returns how many.
LOO_MM_AP_EXPORT int loo_mm_ap_cpu_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                        const double* expo, const double* X, double lambda_mu_mu, const double* a, int s,
                                        double k_threshold, int max_iters, double* out, int* kinds) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  std::vector<int> kd;
  ppcx::loo_mm_ap_cell_host(g, a, s, k_threshold, max_iters, out, &kd);
  for (size_t j = 0; j < kd.size(); ++j) kinds[j] = kd[j];
  return (int)kd.size();
}
// the predictive form of the same cell: out [12 + 2 (C + 1)]
LOO_MM_AP_EXPORT void loo_mm_ap_cpu_exact_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                               const double* expo, const double* X, double lambda_mu_mu, const double* a, int s,
                                               double k_threshold, int max_iters, double tc, double p_lo, double p_hi, double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_ap_exact_cell_host(g, a, s, k_threshold, max_iters, tc, p_lo, p_hi, out);
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
int main() {
  const int C = 2, S = 5, nc = C + 1;
  const int yrow[S] = {120, 180, -96, 160, 900};
  const double expo[S] = {0.0, 0.1, -0.1, 0.05, 0.0}, X[C * S] = {1, 1, 1, 1, 1, 0, 1, 0, 1, 0};
  int matched = 0;
  for (long n : {1L, 20L, 21L, 400L}) {
    std::vector<double> T((size_t)nc * n), U((size_t)6 * n);
    for (long i = 0; i < n; ++i) {
      T[i] = 5.0 + 0.2 * sin((double)i); T[n + i] = 0.1 * cos(2.0 * (double)i); T[2 * n + i] = -1.0 + 0.3 * sin(5.0 * (double)i);
      const double u[6] = {0.5, 0.6, -1.0, -1.2, 0.0, -0.9};
      for (int k = 0; k < 6; ++k) U[k * n + i] = u[k] + 0.01 * sin((double)(i + k));
    }
    for (int kind = 0; kind < 3; ++kind) {                   // the log ratios: clean, with a draw that takes no part, with a NaN
      std::vector<double> a((size_t)n);
      for (long i = 0; i < n; ++i) a[i] = 0.4 * sin(1.3 * (double)i) + 0.2 * cos(0.7 * (double)i * (double)i);
      if (kind == 1) a[n / 2] = -INFINITY;
      if (kind == 2) a[n / 2] = NAN;
      for (int checked = 0; checked < 2; ++checked)
        for (int s : {1, 2, 4}) {
          const ppcx::LooMmGene g = gene_of(T.data(), U.data(), n, C, S, checked, yrow, expo, X, 5.6);
          double out[6 + 2 * nc], ex[12 + 2 * nc];
          std::vector<int> kd;
          ppcx::loo_mm_ap_cell_host(g, a.data(), s, 0.3, 5, out, &kd);
          ppcx::loo_mm_ap_exact_cell_host(g, a.data(), s, 0.3, 5, 1.0, 0.025, 0.975, ex);
          printf("n=%ld a=%d checked=%d s=%d elpd=%.6f khat=%g before=%g iterations=%g scale=%g %g %g shift=%g %g %g mean=%.6f p_le=%g khat=%g\n",
                 n, kind, checked, s, out[0], out[3], out[4], out[5], out[6], out[7], out[8], out[9], out[10], out[11], ex[0], ex[2], ex[9]);
          if ((int)out[5] != (int)kd.size() || ex[11] != out[5]) return 1;
          if (kind == 2 && !(out[0] != out[0] && out[5] == 0.0)) return 1;          // a NaN log ratio: the cell is NaN and unmatched
          for (int k = 0; k < 2 * nc; ++k) if (ex[12 + k] != out[6 + k]) return 1;   // the two forms agree on the state
          if (out[5] > 0.0 && !(ex[9] == out[3] || ex[9] != ex[9])) return 1;        // ... and on the final khat
          matched += out[5] > 0.0;
        }
    }
  }
  printf("cells matched: %d\n", matched);
  return matched > 0 ? 0 : 1;
}
#endif
