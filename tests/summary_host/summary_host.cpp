// CPU build of the fit summary's per-column statistics (ppcseq_amd/csrc/ppcx_summary.h) for tests/test_summary_host.py:
// the same header the gfx950 kernel includes, compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a
// stand-alone program (fixed columns, for a run under -fsanitize=address,undefined: tests/host_build.py).
#include "../../ppcseq_amd/csrc/ppcx_summary.h"

extern "C" __attribute__((visibility("default"))) void summary_host_column(const double* x, int M, int n, double* out, double* ranks) {
  ppcx::summary_column_host(x, M, n, out, ranks);
}
extern "C" __attribute__((visibility("default"))) double summary_host_ndtri(double p) { return ppcx::ndtri(p); }

#ifdef PPCX_HOST_MAIN
#include "../host_main.h"
int main() {
  using namespace host_main;
  const double z = summary_host_ndtri(0.975);
  printf("ndtri(0.5)=%g ndtri(0.975)=%.6f\n", summary_host_ndtri(0.5), z);
  if (summary_host_ndtri(0.5) != 0.0 || !(z > 1.95 && z < 1.97)) return impossible("ndtri at 0.5 and 0.975");
  for (int M : {1, 4})
    for (long n : kDraws)
      for (Kind kind : kKinds) {
        const std::vector<double> x = column((long)M * n, kind, 2.0);
        std::vector<double> ranks((size_t)(2 * M * (n / 2) > 0 ? 2 * M * (n / 2) : 1));
        double out[ppcx::SUM_FIELDS];
        summary_host_column(x.data(), M, (int)n, out, ranks.data());
        printf("chains=%d n=%ld %s mean=%.6f sd=%.6f q05=%.6f q50=%.6f q95=%.6f rhat=%.6f ess_bulk=%.3f ess_tail=%.3f\n", M, n,
               kKindNames[kind], out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7]);
        if (kind != CLEAN) { if (!all_nan(out, ppcx::SUM_FIELDS)) return impossible("a column with a value that is not finite is NaN"); continue; }
        if (!(isfinite(out[ppcx::SUM_MEAN]) && out[ppcx::SUM_Q05] <= out[ppcx::SUM_Q50] && out[ppcx::SUM_Q50] <= out[ppcx::SUM_Q95]))
          return impossible("mean and ordered quantiles of a clean column");
        if (n / 2 >= 2 && !(out[ppcx::SUM_RHAT] > 0.0 && out[ppcx::SUM_ESS_BULK] > 0.0 && out[ppcx::SUM_ESS_TAIL] > 0.0))
          return impossible("R-hat and ESS of split chains of 2 draws or more");
        if (n / 2 < 2 && !(isnan(out[ppcx::SUM_RHAT]) && isnan(out[ppcx::SUM_ESS_BULK]))) return impossible("no split chains, no R-hat");
      }
  return 0;
}
#endif
