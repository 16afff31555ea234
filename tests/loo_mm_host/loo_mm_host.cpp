// CPU build of the gene-local moment matching of PSIS-LOO cells (ppcseq_amd/csrc/ppcx_loo_mm.h) for tests/test_loo_mm_host.py:
// the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a
// stand-alone program (a fixed gene, for a run under -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_mm.h"

#define LOO_MM_EXPORT extern "C" __attribute__((visibility("default")))

static ppcx::LooMmGene gene_of(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow, const double* expo,
                               const double* X, double lambda_mu_mu) {
  ppcx::LooMmGene g;
  g.Tg = T; g.U = U; g.n = n; g.C = C; g.S = S; g.checked = checked != 0; g.yrow = yrow; g.expo = expo; g.X = X;
  g.lambda_mu_mu = lambda_mu_mu;
  return g;
}

// one cell: T [C + 1][n], U [6][n], yrow [S] (an excluded cell as -(y + 1)), expo [S], X [C][S]; out [6 + 2 (C + 1)]; kinds
// [max_iters] receives the accepted candidates (1 or 2) in order. Returns how many.
LOO_MM_EXPORT int loo_mm_host_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                   const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff, double k_threshold,
                                   int max_iters, double* out, int* kinds) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  std::vector<int> kd;
  ppcx::loo_mm_cell_host(g, s, r_eff, k_threshold, max_iters, out, &kd);
  for (size_t j = 0; j < kd.size(); ++j) kinds[j] = kd[j];
  return (int)kd.size();
}
// the local density q [n] and the log-likelihood of cell s [n] at every draw under the state (A, B) [C + 1]
LOO_MM_EXPORT void loo_mm_host_density(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                       const double* expo, const double* X, double lambda_mu_mu, int s, const double* A, const double* B,
                                       double* q, double* ll) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  for (long i = 0; i < n; ++i) q[i] = ppcx::loo_mm_density(g, i, A, B, s, &ll[i]);
}
// plain PSIS-LOO of a column (ppcx_loo.h loo_cell_host), for the bit-for-bit check of the untouched cells: out [4]
LOO_MM_EXPORT void loo_mm_host_loo_cell(const double* ll, long n, double r_eff, int excluded, double* out) {
  ppcx::loo_cell_host(ll, n, r_eff, excluded != 0, out);
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
int main() {
  const int C = 2, S = 5;
  const int yrow[S] = {120, 180, -96, 160, 900};
  const double expo[S] = {0.0, 0.1, -0.1, 0.05, 0.0}, X[C * S] = {1, 1, 1, 1, 1, 0, 1, 0, 1, 0};
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
        double out[6 + 2 * (C + 1)];
        std::vector<int> kd;
        ppcx::loo_mm_cell_host(g, s, 0.8, 0.3, 5, out, &kd);
        printf("n=%ld checked=%d s=%d elpd=%.6f khat=%g before=%g iterations=%g scale=%g %g %g shift=%g %g %g\n", n, checked, s, out[0],
               out[3], out[4], out[5], out[6], out[7], out[8], out[9], out[10], out[11]);
        if ((int)out[5] != (int)kd.size()) return 1;
      }
  }
  return 0;
}
#endif
