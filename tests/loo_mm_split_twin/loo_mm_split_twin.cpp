// CPU build of the split transformation of gene-local moment matching (ppcseq_amd/csrc/ppcx_loo_mm_split.h) for
// tests/test_loo_mm_split_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With
// -DPPCX_HOST_MAIN it is a stand-alone program (a fixed gene, for a run under -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_mm_split.h"

#define LOO_MM_SPLIT_EXPORT extern "C" __attribute__((visibility("default")))

static ppcx::LooMmGene gene_of(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow, const double* expo,
                               const double* X, double lambda_mu_mu) {
  ppcx::LooMmGene g;
  g.Tg = T; g.U = U; g.n = n; g.C = C; g.S = S; g.checked = checked != 0; g.yrow = yrow; g.expo = expo; g.X = X;
  g.lambda_mu_mu = lambda_mu_mu;
  return g;
}

// one cell: T [C + 1][n], U [6][n], yrow [S] (an excluded cell as -(y + 1)), expo [S], X [C][S]; out [8 + 2 (C + 1)]
LOO_MM_SPLIT_EXPORT void loo_mm_split_twin_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                                const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff,
                                                double k_threshold, int max_iters, double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_split_cell_host(g, s, r_eff, k_threshold, max_iters, out);
}
// the same from a given record rec [6 + 2 (C + 1)] of the matching
LOO_MM_SPLIT_EXPORT void loo_mm_split_twin_from_record(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                                       const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff,
                                                       const double* rec, double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_split_from_record_host(g, s, r_eff, rec, out);
}
// the predictive form: out [13 + 2 (C + 1)]
LOO_MM_SPLIT_EXPORT void loo_mm_split_twin_exact_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                                      const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff,
                                                      double k_threshold, int max_iters, double tc, double p_lo, double p_hi, double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_exact_split_cell_host(g, s, r_eff, k_threshold, max_iters, tc, p_lo, p_hi, out);
}
LOO_MM_SPLIT_EXPORT void loo_mm_split_twin_exact_from_record(const double* T, const double* U, long n, int C, int S, int checked,
                                                             const int* yrow, const double* expo, const double* X, double lambda_mu_mu,
                                                             int s, double r_eff, double tc, double p_lo, double p_hi, const double* rec,
                                                             double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_exact_split_from_record_host(g, s, r_eff, tc, p_lo, p_hi, rec, out);
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
int main() {
  const int C = 2, S = 5;
  const int yrow[S] = {120, 180, -96, 160, 900};
  const double expo[S] = {0.0, 0.1, -0.1, 0.05, 0.0}, X[C * S] = {1, 1, 1, 1, 1, 0, 1, 0, 1, 0};
  int split = 0;
  for (long n : {1L, 2L, 3L, 21L, 400L}) {
    std::vector<double> T((C + 1) * n), U(6 * n);
    for (long i = 0; i < n; ++i) {
      T[i] = 5.0 + 0.2 * sin((double)i); T[n + i] = 0.1 * cos(2.0 * (double)i); T[2 * n + i] = -1.0 + 0.3 * sin(5.0 * (double)i);
      const double u[6] = {0.5, 0.6, -1.0, -1.2, 0.0, -0.9};
      for (int k = 0; k < 6; ++k) U[k * n + i] = u[k] + 0.01 * sin((double)(i + k));
    }
    for (int checked = 0; checked < 2; ++checked)
      for (int s : {1, 2, 4}) {
        const ppcx::LooMmGene g = gene_of(T.data(), U.data(), n, C, S, checked, yrow, expo, X, 5.6);
        double out[8 + 2 * (C + 1)], ex[13 + 2 * (C + 1)];
        ppcx::loo_mm_split_cell_host(g, s, 0.8, 0.3, 5, out);
        ppcx::loo_mm_exact_split_cell_host(g, s, 0.8, 0.3, 5, 0.7352941, 0.025, 0.975, ex);
        printf("n=%ld checked=%d s=%d elpd_loo=%.6f matched=%.6f khat=%g khat_split=%g iterations=%g | mean=%.6f lower=%g upper=%g khat_split=%g\n",
               n, checked, s, out[0], out[6 + 2 * (C + 1)], out[3], out[7 + 2 * (C + 1)], out[5], ex[0], ex[4], ex[5], ex[12 + 2 * (C + 1)]);
        split += out[5] > 0.0;
        if (out[5] != ex[11]) return 1;
        if (ex[4] > ex[5]) return 1;
        // a record of one accepted step that moved nothing: the ratios are -ll - ln 2
        double rec[6 + 2 * (C + 1)];
        for (int c = 0; c < 6 + 2 * (C + 1); ++c) rec[c] = out[c];
        rec[5] = 1.0;
        for (int c = 0; c <= C; ++c) { rec[6 + c] = 1.0; rec[6 + C + 1 + c] = 0.0; }
        ppcx::loo_mm_split_from_record_host(g, s, 0.8, rec, out);
        ppcx::loo_mm_exact_split_from_record_host(g, s, 0.8, 0.7352941, 0.025, 0.975, rec, ex);
      }
  }
  printf("split cells: %d\n", split);
  return split > 0 ? 0 : 1;
}
#endif
