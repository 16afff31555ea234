// CPU build of the Pareto-k diagnostic (ppcseq_amd/csrc/ppcx_psis.h) for tests/test_psis_host.py: the same header the gfx950
// kernel includes, compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (fixed columns,
// for a run under -fsanitize=address,undefined: tests/host_build.py).
#include "../../ppcseq_amd/csrc/ppcx_psis.h"

extern "C" __attribute__((visibility("default"))) double psis_host_khat(const double* v, long n) { return ppcx::psis_khat_host(v, n); }

#ifdef PPCX_HOST_MAIN
#include "../host_main.h"
int main() {
  using namespace host_main;
  for (long n : kDraws)
    for (Kind kind : kKinds) {
      const std::vector<double> v = column(n, kind);
      const double k = psis_host_khat(v.data(), n);
      printf("n=%ld %s khat=%g\n", n, kKindNames[kind], k);
      if (isnan(k) != (kind == WITH_NAN)) return impossible("k-hat is NaN exactly for a column with a NaN");
      const long N = n - (kind == WITH_MINUS_INF);                 // a -Inf ratio takes no part
      if (kind != WITH_NAN && N <= 20 && k != INFINITY) return impossible("a tail below 5 values has k-hat Inf");
      if (kind != WITH_NAN && N > 20 && !isfinite(k)) return impossible("a smooth tail of 5 values or more has a finite k-hat");
    }
  return 0;
}
#endif
