// CPU build of the relative efficiency per cell (ppcseq_amd/csrc/ppcx_reff.h) for tests/test_reff_host.py: the same header the
// gfx950 kernel includes, compiled with g++ and called through ctypes. With -DPPCX_HOST_MAIN it is a stand-alone program (fixed
// columns, for a run under -fsanitize=address,undefined: tests/host_build.py).
#include "../../ppcseq_amd/csrc/ppcx_reff.h"

extern "C" __attribute__((visibility("default"))) double reff_host_cell(const double* ll, int M, int n) {
  return ppcx::relative_eff_cell_host(ll, M, n);
}

#ifdef PPCX_HOST_MAIN
#include "../host_main.h"
int main() {
  using namespace host_main;
  for (int M : {1, 4})
    for (long n : kDraws)
      for (Kind kind : kKinds) {
        const std::vector<double> ll = column((long)M * n, kind);
        const double r = reff_host_cell(ll.data(), M, (int)n);
        printf("chains=%d n=%ld %s r_eff=%.6f\n", M, n, kKindNames[kind], r);
        // the NaN sits at (M n) / 2: the middle draw that an odd n drops when there is one chain, a split value otherwise
        const bool nan_in_split = kind == WITH_NAN && !(M == 1 && n % 2 == 1);
        if (n / 2 < 2 || nan_in_split ? !isnan(r) : !(r > 0.0 && isfinite(r)))
          return impossible("r_eff is NaN below 2 draws per split chain or with a NaN among the split values, else positive");
      }
  return 0;
}
#endif
