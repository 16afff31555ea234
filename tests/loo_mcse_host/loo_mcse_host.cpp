// CPU build of PSIS-LOO per cell with the Monte-Carlo standard error and n_eff (ppcseq_amd/csrc/ppcx_loo.h steps 5 - 8) for
// tests/test_loo_mcse_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_loo.h"

extern "C" __attribute__((visibility("default"))) void loo_mcse_host_cell(const double* ll, long n, double r_eff, int excluded,
                                                                          double* out) {
  ppcx::loo_cell_host(ll, n, r_eff, excluded != 0, out, true);
}
