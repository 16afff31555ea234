// CPU build of the exact leave-one-out predictive under the weights of the matching with the covariance step
// (ppcseq_amd/csrc/ppcx_loo_mm_cov_exact.h) for tests/test_loo_mm_cov_exact_host.py: the same header the gfx950 kernel includes,
// compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (fixed genes, for a run under
// -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_mm_cov_exact.h"

#define LOO_MM_COV_EXACT_EXPORT extern "C" __attribute__((visibility("default")))

static ppcx::LooMmGene gene_of(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow, const double* expo,
                               const double* X, double lambda_mu_mu) {
  ppcx::LooMmGene g;
  g.Tg = T; g.U = U; g.n = n; g.C = C; g.S = S; g.checked = checked != 0; g.yrow = yrow; g.expo = expo; g.X = X;
  g.lambda_mu_mu = lambda_mu_mu;
  return g;
}

// one cell: T [C + 1][n], U [6][n], yrow [S] (an excluded cell as -(y + 1)), expo [S], X [C][S]; out [14 + (C + 1)^2 + (C + 1)]
LOO_MM_COV_EXACT_EXPORT void loo_mm_cov_exact_cpu_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                                       const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff,
                                                       double k_threshold, int max_iters, int split, double tc, double p_lo, double p_hi,
                                                       double* out) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  ppcx::loo_mm_cov_exact_cell_host(g, s, r_eff, k_threshold, max_iters, split != 0, tc, p_lo, p_hi, out);
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
// fixed genes at d = 5 (C = 4) and d = 17 (C = 16): n = d, d + 1 and a few hundred, split on and off; a path with a covariance
// step must occur at either width
template <int C, int S>
static int run(const int* yrow, const double* expo, const double* X, const long* ns, int n_ns, const int* cells, int n_cells, double slope0) {
  const int nc = C + 1;
  int cov = 0;
  for (int q = 0; q < n_ns; ++q) {
    const long n = ns[q];
    std::vector<double> T((size_t)nc * n), U((size_t)6 * n);
    for (long i = 0; i < n; ++i) {
      const double x = (double)i;
      T[i] = 5.0 + 0.2 * sin(x) + 0.1 * cos(3.0 * x);
      for (int c = 1; c < C; ++c) T[c * n + i] = 0.1 * sin((2.0 + 0.7 * c) * x + c) + (slope0 - 0.04 * c) * (T[i] - 5.0);
      T[C * n + i] = -1.0 + 0.3 * sin(5.0 * x) - 0.4 * (T[i] - 5.0);
      const double u[6] = {0.5, 0.6, -1.0, -1.2, 0.0, -0.9};
      for (int k = 0; k < 6; ++k) U[k * n + i] = u[k] + 0.01 * sin((double)(i + k));
    }
    for (int j = 0; j < n_cells; ++j)
      for (int split = 0; split < 2; ++split) {
        const int s = cells[j];
        const ppcx::LooMmGene g = gene_of(T.data(), U.data(), n, C, S, 1, yrow, expo, X, 5.6);
        double out[14 + nc * nc + nc];
        ppcx::loo_mm_cov_exact_cell_host(g, s, 0.8, 0.1, 6, split != 0, 1.0, 0.025, 0.975, out);
        printf("C=%d n=%ld s=%d split=%d mean=%.6f sd=%.6f p_le=%g p_ge=%g lower=%g upper=%g khat=%g khat_split=%g iterations=%g cov=%g\n",
               C, n, s, split, out[0], out[1], out[2], out[3], out[4], out[5], out[9], out[13], out[11], out[12]);
        cov += out[12] > 0.0;
        if (n <= nc && out[12] != 0.0) return -1;                              // n <= d: candidate 3 is refused
        if (!(out[13] == out[13]) != (!split || out[11] == 0.0 || !(out[0] == out[0]))) return -1;   // khat_split is NaN exactly there
        for (int k = 0; k < nc * nc + nc; ++k) if (!(out[14 + k] == out[14 + k])) return -1;       // never a NaN state
      }
  }
  return cov;
}

int main() {
  const long n5[] = {5, 6, 700}, n17[] = {17, 18, 300};
  const int S5 = 6, C5 = 4;
  const int y5[S5] = {120, 180, -96, 160, 2500, 140};
  const double e5[S5] = {0.0, 0.1, -0.1, 0.05, 0.0, 0.02};
  double X5[C5 * S5] = {0.0};
  for (int s = 0; s < S5; ++s) { X5[s] = 1.0; if (s % C5) X5[(s % C5) * S5 + s] = 1.0; }
  const int cells5[] = {1, 2, 4};
  const int cov5 = run<C5, S5>(y5, e5, X5, n5, 3, cells5, 3, 0.3);
  const int CW = 16, SW = 20;
  int yw[SW];
  double ew[SW], XW[CW * SW] = {0.0};
  for (int s = 0; s < SW; ++s) { yw[s] = 150 + 37 * (s % 5); ew[s] = 0.01 * s; XW[s] = 1.0; if (s % CW) XW[(s % CW) * SW + s] = 1.0; }
  yw[5] = 1500; yw[3] = -201;
  const int cellsw[] = {3, 5, 19};
  const int covw = run<CW, SW>(yw, ew, XW, n17, 3, cellsw, 3, 0.3);
  printf("cells with a covariance step: d = 5: %d, d = 17: %d\n", cov5, covw);
  return cov5 > 0 && covw > 0 ? 0 : 1;
}
#endif
