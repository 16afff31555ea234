// CPU build of the fit summary's per-column statistics (ppcseq_amd/csrc/ppcx_summary.h) for tests/test_summary_host.py:
// the same header the gfx950 kernel includes, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_summary.h"

extern "C" __attribute__((visibility("default"))) void summary_host_column(const double* x, int M, int n, double* out, double* ranks) {
  ppcx::summary_column_host(x, M, n, out, ranks);
}
extern "C" __attribute__((visibility("default"))) double summary_host_ndtri(double p) { return ppcx::ndtri(p); }
