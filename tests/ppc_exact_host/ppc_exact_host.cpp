// CPU build of the exact posterior-predictive tails and interval per cell (ppcseq_amd/csrc/ppcx_nbcdf.h, ppcx_ppc_exact.h) for
// tests/test_nbcdf_host.py and tests/test_ppc_exact_host.py: the same headers the gfx950 kernel includes, compiled with g++ and
// called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (a fixed set of points and cells, for a run under
// -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_ppc_exact.h"

#define PPC_EXACT_EXPORT extern "C" __attribute__((visibility("default")))

// p_le, p_ge and the continued fraction's steps at n points
PPC_EXACT_EXPORT void ppc_exact_host_tails(int n, const int32_t* y, const double* eta, const double* phi, double* p_le, double* p_ge,
                                           int32_t* iters) {
  for (int i = 0; i < n; ++i) iters[i] = ppcx::nb2_log_tails(y[i], eta[i], phi[i], &p_le[i], &p_ge[i]);
}
// one cell: out[kPpcExactFields]; returns the largest number of continued-fraction steps
PPC_EXACT_EXPORT int ppc_exact_host_cell(const double* eta, const double* sigma_raw, long n, int y, int excluded, double tc,
                                         double p_lo, double p_hi, double* out) {
  int mx = 0;
  ppcx::ppc_exact_cell_host(eta, sigma_raw, n, y, excluded != 0, tc, p_lo, p_hi, out, &mx);
  return mx;
}
// the host build of the predictive sampler (ppcx_math.h nb2_log_rng), for the consistency check with counts_rng
PPC_EXACT_EXPORT void ppc_exact_host_rng(int n, const double* eta, const double* phi, uint32_t k0, uint32_t cell, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = ppcx::nb2_log_rng(eta[i], phi[i], k0, cell, (uint32_t)i);
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
#include <vector>
int main() {
  const int ys[] = {0, 1, 2, 7, 8, 667, 2001, 100000, 2580228};
  const double phis[] = {1e-3, 0.5, 5.0, 100.0, 1e5}, mus[] = {0.01, 5.0, 667.0, 1e5, 2.6e6};
  int worst = 0;
  for (int y : ys) for (double phi : phis) for (double mu : mus) {
    double a, b;
    const int it = ppcx::nb2_log_tails(y, log(mu), phi, &a, &b);
    worst = it > worst ? it : worst;
    if (!(a >= 0.0 && a <= 1.0 && b >= 0.0 && b <= 1.0 + 1e-12)) { printf("bad tails at y=%d phi=%g mu=%g: %g %g\n", y, phi, mu, a, b); return 1; }
  }
  for (long n : {1L, 20L, 1000L}) {
    std::vector<double> eta(n), sg(n);
    for (long i = 0; i < n; ++i) { eta[i] = 5.0 + 0.3 * sin((double)i); sg[i] = -1.0 + 0.2 * cos(3.0 * (double)i); }
    double out[ppcx::kPpcExactFields]; int mx = 0;
    ppcx::ppc_exact_cell_host(eta.data(), sg.data(), n, 140, false, 0.7352941, 2.4e-4, 1.0 - 2.4e-4, out, &mx);
    worst = mx > worst ? mx : worst;
    printf("n=%ld mean=%.6f sd=%.6f p_le=%.6g p_ge=%.6g lower=%g upper=%g\n", n, out[0], out[1], out[2], out[3], out[4], out[5]);
    if (!(out[4] <= out[5])) return 1;
  }
  printf("largest continued-fraction step count: %d\n", worst);
  return 0;
}
#endif
