// CPU build of PSIS-LOO per cell of an ADVI fit (ppcseq_amd/csrc/ppcx_loo_ap.h) for tests/test_loo_ap_host.py: the same header
// the gfx950 kernels include, compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (fixed
// columns, for a run under -fsanitize=address,undefined: tests/host_build.py).
#include "../../ppcseq_amd/csrc/ppcx_loo_ap.h"

extern "C" __attribute__((visibility("default"))) void loo_ap_host_cell(const double* ll, const double* log_ratio, long n,
                                                                        int excluded, double* out) {
  ppcx::loo_ap_cell_host(ll, log_ratio, n, excluded != 0, out);
}

#ifdef PPCX_HOST_MAIN
#include "../host_main.h"
int main() {
  using namespace host_main;
  for (long n : kDraws)
    for (Kind kind : kKinds)
      for (Kind ratio_kind : kKinds)                        // the fit's log ratios p / g: clean, with a NaN, with a draw that takes no part
        for (int excluded = 0; excluded < 2; ++excluded) {
          if (n == 1 && kind == WITH_MINUS_INF && ratio_kind == WITH_MINUS_INF) continue;      // -Inf + Inf: not a stated case
          const std::vector<double> ll = column(n, kind);
          std::vector<double> a = column(n, CLEAN, 0.0, 1.0);
          if (ratio_kind != CLEAN) a[0] = ratio_kind == WITH_NAN ? NAN : -INFINITY;           // ll's is the middle draw
          double out[ppcx::kLooFields];
          loo_ap_host_cell(ll.data(), a.data(), n, excluded, out);
          printf("n=%ld ll %s ratio %s excluded=%d elpd_loo=%.6f p_loo=%.6f looic=%.6f khat=%g\n", n, kKindNames[kind],
                 kKindNames[ratio_kind], excluded, out[0], out[1], out[2], out[3]);
          // ll = -Inf in a cell that takes part is a ratio +Inf; a ratio -Inf takes no part, which at n = 1 leaves no draw
          const bool nan = kind == WITH_NAN || ratio_kind == WITH_NAN || (kind == WITH_MINUS_INF && !excluded) ||
                           (ratio_kind == WITH_MINUS_INF && n == 1);
          if (nan) { if (!all_nan(out, ppcx::kLooFields)) return impossible("a NaN, a ratio +Inf or no draw makes the cell NaN"); continue; }
          if (!(!isnan(out[0]) && out[2] == -2.0 * out[0])) return impossible("elpd_loo is a number and looic = -2 elpd_loo");
          if (isnan(out[3]) || (excluded && out[1] != 0.0)) return impossible("k-hat is a number; an excluded cell has p_loo 0");
        }
  return 0;
}
#endif
