// CPU build of the Pareto-k diagnostic (ppcseq_amd/csrc/ppcx_psis.h) for tests/test_psis_host.py: the same header the gfx950
// kernel includes, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_psis.h"

extern "C" __attribute__((visibility("default"))) double psis_host_khat(const double* v, long n) { return ppcx::psis_khat_host(v, n); }
