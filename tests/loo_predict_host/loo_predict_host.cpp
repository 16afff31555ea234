// CPU build of the leave-one-out predictive interval per cell (ppcseq_amd/csrc/ppcx_loo_predict.h) for
// tests/test_loo_predict_host.py: the same header the gfx950 kernel includes, compiled with g++ and called through ctypes.
#include "../../ppcseq_amd/csrc/ppcx_loo_predict.h"

extern "C" __attribute__((visibility("default"))) void loo_predict_host_cell(const double* ll, const int32_t* x, long n, int y,
                                                                             double r_eff, int excluded, double p_lo, double p_hi,
                                                                             double* out) {
  ppcx::loo_predict_cell_host(ll, x, n, y, r_eff, excluded != 0, p_lo, p_hi, out);
}
