// CPU build of PSIS-LOO per cell (ppcseq_amd/csrc/ppcx_loo.h) for tests/test_loo_host.py: the same header the gfx950 kernel
// includes, compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (fixed columns, for a
// run under -fsanitize=address,undefined: tests/host_build.py).
#include "../../ppcseq_amd/csrc/ppcx_loo.h"

extern "C" __attribute__((visibility("default"))) void loo_host_cell(const double* ll, long n, double r_eff, int excluded,
                                                                     double* out) {
  ppcx::loo_cell_host(ll, n, r_eff, excluded != 0, out);
}

#ifdef PPCX_HOST_MAIN
#include "../host_main.h"
int main() {
  using namespace host_main;
  for (long n : kDraws)
    for (Kind kind : kKinds)
      for (int excluded = 0; excluded < 2; ++excluded) {
        const std::vector<double> ll = column(n, kind);
        double out[ppcx::kLooFields];
        loo_host_cell(ll.data(), n, 0.8, excluded, out);
        printf("n=%ld %s excluded=%d elpd_loo=%.6f p_loo=%.6f looic=%.6f khat=%g\n", n, kKindNames[kind], excluded, out[0], out[1], out[2],
               out[3]);
        if (kind == WITH_NAN || (kind == WITH_MINUS_INF && !excluded)) {
          if (!all_nan(out, ppcx::kLooFields)) return impossible("a NaN, or a -Inf in a cell that takes part, makes the cell NaN");
          continue;
        }
        if (!(!isnan(out[0]) && out[2] == -2.0 * out[0])) return impossible("elpd_loo is a number and looic = -2 elpd_loo");
        if (excluded ? !(out[1] == 0.0 && isnan(out[3])) : isnan(out[3])) return impossible("an excluded cell has p_loo 0 and no k-hat");
        if (!excluded && n <= 20 && out[3] != INFINITY) return impossible("a tail below 5 values has k-hat Inf");
      }
  return 0;
}
#endif
