// CPU build of the relative efficiency per cell (ppcseq_amd/csrc/ppcx_reff.h) for tests/test_reff_host.py: the same header the
// gfx950 kernel includes, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_reff.h"

extern "C" __attribute__((visibility("default"))) double reff_host_cell(const double* ll, int M, int n) {
  return ppcx::relative_eff_cell_host(ll, M, n);
}
