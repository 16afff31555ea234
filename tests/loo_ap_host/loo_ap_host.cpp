// CPU build of PSIS-LOO per cell of an ADVI fit (ppcseq_amd/csrc/ppcx_loo_ap.h) for tests/test_loo_ap_host.py: the same header
// the gfx950 kernels include, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_loo_ap.h"

extern "C" __attribute__((visibility("default"))) void loo_ap_host_cell(const double* ll, const double* log_ratio, long n,
                                                                        int excluded, double* out) {
  ppcx::loo_ap_cell_host(ll, log_ratio, n, excluded != 0, out);
}
