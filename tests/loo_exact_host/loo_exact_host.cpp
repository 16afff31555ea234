// CPU build of the exact leave-one-out predictive tails and interval per cell (ppcseq_amd/csrc/ppcx_loo_exact.h) for
// tests/test_loo_exact_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With
// -DPPCX_HOST_MAIN it is a stand-alone program (a fixed set of cells, for a run under -fsanitize=address,undefined).
#include "../../ppcseq_amd/csrc/ppcx_loo_exact.h"

#define LOO_EXACT_EXPORT extern "C" __attribute__((visibility("default")))

// one cell: out[kLooExactFields]; log_ratio null (a NUTS fit) or [n]; returns the largest number of continued-fraction steps
LOO_EXACT_EXPORT int loo_exact_host_cell(const double* ll, const double* eta, const double* sigma_raw, const double* log_ratio, long n,
                                         int y, int excluded, double r_eff, double tc, double p_lo, double p_hi, double* out) {
  int mx = 0;
  ppcx::loo_exact_cell_host(ll, eta, sigma_raw, log_ratio, n, y, excluded != 0, r_eff, tc, p_lo, p_hi, out, &mx);
  return mx;
}
// the posterior-predictive cell of ppcx_ppc_exact.h, for the bit-for-bit check of an excluded cell: out[kPpcExactFields]
LOO_EXACT_EXPORT void loo_exact_host_ppc_cell(const double* eta, const double* sigma_raw, long n, int y, int excluded, double tc,
                                              double p_lo, double p_hi, double* out) {
  ppcx::ppc_exact_cell_host(eta, sigma_raw, n, y, excluded != 0, tc, p_lo, p_hi, out);
}
// the cell's own log-pmf at every draw, ln phi = -sigma_raw (no truncation compensation): ll as a fit forms it up to rounding
LOO_EXACT_EXPORT void loo_exact_host_log_pmf(const double* eta, const double* sigma_raw, long n, int y, double* ll) {
  for (long i = 0; i < n; ++i) ll[i] = ppcx::loo_ll(y, eta[i], sigma_raw[i]);
}

#ifdef PPCX_HOST_MAIN
#include <stdio.h>
#include <vector>
int main() {
  int worst = 0;
  for (long n : {1L, 20L, 1000L}) {
    std::vector<double> eta(n), sg(n), ll(n), lr(n);
    for (long i = 0; i < n; ++i) {
      eta[i] = 5.0 + 0.3 * sin((double)i); sg[i] = -1.0 + 0.2 * cos(3.0 * (double)i);
      ll[i] = ppcx::loo_ll(140, eta[i], sg[i]); lr[i] = 0.5 * sin(7.0 * (double)i);
    }
    for (int form = 0; form < 4; ++form) {               // NUTS / ADVI, excluded or not
      double out[ppcx::kLooExactFields]; int mx = 0;
      ppcx::loo_exact_cell_host(ll.data(), eta.data(), sg.data(), form & 1 ? lr.data() : nullptr, n, 140, (form & 2) != 0, 0.7, 0.7352941,
                                2.4e-4, 1.0 - 2.4e-4, out, &mx);
      worst = mx > worst ? mx : worst;
      printf("n=%ld form=%d mean=%.6f sd=%.6f p_le=%.6g p_ge=%.6g lower=%g upper=%g khat=%g\n", n, form, out[0], out[1], out[2], out[3],
             out[4], out[5], out[9]);
      if (!(out[4] <= out[5])) return 1;
    }
  }
  printf("largest continued-fraction step count: %d\n", worst);
  return 0;
}
#endif
