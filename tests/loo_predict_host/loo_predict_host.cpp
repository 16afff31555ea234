// CPU build of the leave-one-out predictive interval per cell (ppcseq_amd/csrc/ppcx_loo_predict.h) for
// tests/test_loo_predict_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With
// -DPPCX_HOST_MAIN it is a stand-alone program (fixed columns, for a run under -fsanitize=address,undefined: tests/host_build.py).
#include "../../ppcseq_amd/csrc/ppcx_loo_predict.h"

extern "C" __attribute__((visibility("default"))) void loo_predict_host_cell(const double* ll, const int32_t* x, long n, int y,
                                                                             double r_eff, int excluded, double p_lo, double p_hi,
                                                                             double* out) {
  ppcx::loo_predict_cell_host(ll, x, n, y, r_eff, excluded != 0, p_lo, p_hi, out);
}

#ifdef PPCX_HOST_MAIN
#include "../host_main.h"
int main() {
  using namespace host_main;
  for (long n : kDraws)
    for (Kind kind : kKinds)
      for (int excluded = 0; excluded < 2; ++excluded) {
        const std::vector<double> ll = column(n, kind);
        const std::vector<int32_t> x = counts(n);
        double out[ppcx::kLooPredictFields];
        loo_predict_host_cell(ll.data(), x.data(), n, 110, 0.8, excluded, 0.025, 0.975, out);
        printf("n=%ld %s excluded=%d mean=%.6f lower=%.6f upper=%.6f pit_lt=%.6f pit_le=%.6f khat=%g\n", n, kKindNames[kind], excluded,
               out[0], out[1], out[2], out[3], out[4], out[5]);
        if (kind == WITH_NAN || (kind == WITH_MINUS_INF && !excluded)) {
          if (!all_nan(out, ppcx::kLooPredictFields)) return impossible("a NaN, or a -Inf in a cell that takes part, makes the cell NaN");
          continue;
        }
        if (!(out[1] <= out[0] && out[0] <= out[2])) return impossible("lower <= mean <= upper at 2.5 % and 97.5 %");
        if (!(0.0 <= out[3] && out[3] <= out[4] && out[4] <= 1.0 + 1e-12)) return impossible("0 <= pit_lt <= pit_le <= 1");
        if (isnan(out[5]) != (excluded != 0)) return impossible("k-hat is NaN exactly for an excluded cell");
      }
  return 0;
}
#endif
