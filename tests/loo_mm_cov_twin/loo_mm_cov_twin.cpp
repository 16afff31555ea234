// CPU build of gene-local moment matching with the covariance step (ppcseq_amd/csrc/ppcx_loo_mm_cov.h) for
// tests/test_loo_mm_cov_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With
// -DPPCX_HOST_MAIN it is a stand-alone program (fixed genes, for a run under -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_mm_cov.h"

#define LOO_MM_COV_EXPORT extern "C" __attribute__((visibility("default")))

static ppcx::LooMmGene gene_of(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow, const double* expo,
                               const double* X, double lambda_mu_mu) {
  ppcx::LooMmGene g;
  g.Tg = T; g.U = U; g.n = n; g.C = C; g.S = S; g.checked = checked != 0; g.yrow = yrow; g.expo = expo; g.X = X;
  g.lambda_mu_mu = lambda_mu_mu;
  return g;
}

// one cell: T [C + 1][n], U [6][n], yrow [S] (an excluded cell as -(y + 1)), expo [S], X [C][S]; out [9 + (C + 1)^2 + (C + 1)];
// kinds [max(1, max_iters)]: the accepted candidates, their number returned; inv [(C + 1)^2 + (C + 1) + 1]: Minv, binv, logJ
LOO_MM_COV_EXPORT int loo_mm_cov_twin_cell(const double* T, const double* U, long n, int C, int S, int checked, const int* yrow,
                                           const double* expo, const double* X, double lambda_mu_mu, int s, double r_eff,
                                           double k_threshold, int max_iters, int split, double* out, int* kinds, double* inv) {
  const ppcx::LooMmGene g = gene_of(T, U, n, C, S, checked, yrow, expo, X, lambda_mu_mu);
  std::vector<int> ks;
  ppcx::loo_mm_cov_cell_host(g, s, r_eff, k_threshold, max_iters, split != 0, out, &ks, inv);
  for (size_t j = 0; j < ks.size(); ++j) kinds[j] = ks[j];
  return (int)ks.size();
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
// fixed columns: n = 1, n = d, n = d + 1, longer ones; a checked gene (d = 4), an unchecked one (d = 2) and a gene whose two slope
// rows are the same column (a singular Sigma and Sigma_w); then 17 coordinates
int main() {
  const int C = 3, S = 5, nc = C + 1;
  const int yrow[S] = {120, 180, -96, 160, 2500};
  const double expo[S] = {0.0, 0.1, -0.1, 0.05, 0.0};
  const double X[C * S] = {1, 1, 1, 1, 1, 0, 1, 0, 1, 0, -1.2, 0.3, 0.6, -0.5, 0.8};
  int matched = 0, cov = 0;
  for (long n : {1L, 2L, 4L, 5L, 21L, 400L}) {
    std::vector<double> T(nc * n), U(6 * n);
    for (int dup = 0; dup < 2; ++dup) {
      for (long i = 0; i < n; ++i) {
        const double x = (double)i;
        T[i] = 5.0 + 0.2 * sin(x) + 0.1 * cos(3.0 * x);
        T[n + i] = 0.1 * cos(2.0 * x) - 0.5 * (T[i] - 5.0);
        T[2 * n + i] = dup ? T[n + i] : 0.05 * sin(7.0 * x) + 0.3 * (T[i] - 5.0);
        T[3 * n + i] = -1.0 + 0.3 * sin(5.0 * x) - 0.4 * (T[i] - 5.0);
        const double u[6] = {0.5, 0.6, -1.0, -1.2, 0.0, -0.9};
        for (int k = 0; k < 6; ++k) U[k * n + i] = u[k] + 0.01 * sin((double)(i + k));
      }
      for (int checked = 0; checked < 2; ++checked)
        for (int s : {1, 2, 4})
          for (int split = 0; split < 2; ++split) {
            const ppcx::LooMmGene g = gene_of(T.data(), U.data(), n, C, S, checked, yrow, expo, X, 5.6);
            double out[9 + nc * nc + nc], inv[nc * nc + nc + 1];
            std::vector<int> kinds;
            ppcx::loo_mm_cov_cell_host(g, s, 0.8, 0.1, 6, split != 0, out, &kinds, inv);
            printf("n=%ld dup=%d checked=%d s=%d split=%d elpd_loo=%.6f matched=%.6f khat=%g khat_split=%g iterations=%g cov=%g kinds",
                   n, dup, checked, s, split, out[0], out[7], out[3], out[8], out[5], out[6]);
            for (int k : kinds) printf(" %d", k);
            printf("\n");
            matched += out[5] > 0.0;
            cov += out[6] > 0.0;
            if ((int)kinds.size() != (int)out[5]) return 1;
            if (n <= (checked ? nc : 2) && out[6] != 0.0) return 1;          // n <= d: candidate 3 is refused
            for (int j = 0; j < nc * nc + nc; ++j) if (out[5] > 0.0 && !(out[9 + j] == out[9 + j])) return 1;   // never a NaN state
          }
    }
  }
  printf("matched cells: %d, with a covariance step: %d\n", matched, cov);
  // the widest design, C = kMaxC = 16 (nc = 17): ones and fifteen indicators, sample s in level s % 16; n = d - 1, d, d + 1, longer
  const int CW = 16, SW = 20, nw = CW + 1;
  int yw[SW];
  double ew[SW], XW[CW * SW] = {0.0};
  for (int s = 0; s < SW; ++s) { yw[s] = 150 + 37 * (s % 5); ew[s] = 0.01 * s; XW[s] = 1.0; if (s % CW) XW[(s % CW) * SW + s] = 1.0; }
  yw[5] = 1500; yw[3] = -201;
  int wide_cov = 0;
  for (long n : {16L, 17L, 18L, 300L}) {
    std::vector<double> T(nw * n), U(6 * n);
    for (long i = 0; i < n; ++i) {
      const double x = (double)i;
      T[i] = 5.0 + 0.2 * sin(x) + 0.1 * cos(3.0 * x);
      for (int c = 1; c < CW; ++c) T[c * n + i] = 0.1 * sin((2.0 + 0.7 * c) * x + c) + (0.3 - 0.04 * c) * (T[i] - 5.0);
      T[CW * n + i] = -1.0 + 0.3 * sin(5.0 * x) - 0.4 * (T[i] - 5.0);
      const double u[6] = {0.5, 0.6, -1.0, -1.2, 0.0, -0.9};
      for (int k = 0; k < 6; ++k) U[k * n + i] = u[k] + 0.01 * sin((double)(i + k));
    }
    for (int checked = 0; checked < 2; ++checked)
      for (int s : {3, 5, 19})
        for (int split = 0; split < 2; ++split) {
          const ppcx::LooMmGene g = gene_of(T.data(), U.data(), n, CW, SW, checked, yw, ew, XW, 5.6);
          double out[9 + nw * nw + nw], inv[nw * nw + nw + 1];
          std::vector<int> kinds;
          ppcx::loo_mm_cov_cell_host(g, s, 0.8, 0.1, 6, split != 0, out, &kinds, inv);
          printf("C=16 n=%ld checked=%d s=%d split=%d elpd_loo=%.6f khat=%g iterations=%g cov=%g\n", n, checked, s, split, out[0], out[3],
                 out[5], out[6]);
          wide_cov += checked && out[6] > 0.0;
          if (n <= (checked ? nw : 2) && out[6] != 0.0) return 1;
          for (int j = 0; j < nw * nw + nw; ++j) if (out[5] > 0.0 && !(out[9 + j] == out[9 + j])) return 1;
        }
  }
  printf("C = 16: checked-gene cells with a covariance step: %d\n", wide_cov);
  return matched > 0 && cov > 0 && wide_cov > 0 ? 0 : 1;
}
#endif
