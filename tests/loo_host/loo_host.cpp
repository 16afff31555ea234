// CPU build of PSIS-LOO per cell (ppcseq_amd/csrc/ppcx_loo.h) for tests/test_loo_host.py: the same header the gfx950 kernel
// includes, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_loo.h"

extern "C" __attribute__((visibility("default"))) void loo_host_cell(const double* ll, long n, double r_eff, int excluded,
                                                                     double* out) {
  ppcx::loo_cell_host(ll, n, r_eff, excluded != 0, out);
}
