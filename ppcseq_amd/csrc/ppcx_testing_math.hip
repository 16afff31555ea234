// ppcx_testing_math.hip -- TESTING BUILD ONLY (-DPPCX_TESTING; ppcseq_amd/build.py adds this translation unit to the testing
// library and to nothing else): the device's scalar building blocks one element at a time, so that tests/ can compare each of
// them with a high-precision reference at the places where such code goes wrong (binade and bin edges, table ends, underflow).
// Every function is the inline one the kernels call (ppcx_math.h, ppcx_model.h), on the device, with the gfx950 assembly of the
// cells enabled; the two log tables are staged in LDS from the host's fill, as the log-likelihood kernel stages them.
#include <hip/hip_runtime.h>
#include <vector>
#include "ppcx_model.h"
#include "ppcx_nbcdf.h"
#include "ppcx_testing.h"

namespace ppcx {

constexpr int kMathThreads = 256;

__global__ __launch_bounds__(kMathThreads) void ppcx_testing_math_kernel(int fn, int n, const double* a, const double* b, const int* y,
                                                                         const double* logtab, const double* wintab, double* out0,
                                                                         double* out1) {
  __shared__ double s_tab[2 * kLogTabSize];
  __shared__ __attribute__((aligned(16))) double s_win[2 * kWinTabSize];
  for (int t = threadIdx.x; t < 2 * kLogTabSize; t += kMathThreads) s_tab[t] = logtab[t];
  for (int t = threadIdx.x; t < 2 * kWinTabSize; t += kMathThreads) s_win[t] = wintab[t];
  __syncthreads();
  const int i = blockIdx.x * kMathThreads + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], x2 = b[i];
  double r0 = 0.0, r1 = 0.0;
  GeneParams<2> gp;
  gp.coef[0] = gp.coef[1] = 0.0; gp.sigma_raw = 0.0; gp.phi = 1.0; gp.invphi = 1.0;
  CellAcc<2> acc; acc.zero();
  switch (fn) {
    case PPCX_MATH_FAST_RCP: r0 = fast_rcp(x); break;
    case PPCX_MATH_FAST_LOG: r0 = fast_log(x); break;
    case PPCX_MATH_FAST_EXP: r0 = fast_exp(x); break;
    case PPCX_MATH_TABLE_LOG: r0 = table_log(x, s_tab); break;
    case PPCX_MATH_WINDOW_LOG: r0 = window_log(x, s_win); break;
    case PPCX_MATH_STIRLING_TAILS: stirling_tails(x, &r0, &r1); break;
    case PPCX_MATH_STIRLING_EXCESS: stirling_excess(x, x2, s_tab, y[i] != 0, &r0, &r1); break;
    case PPCX_MATH_LOG_ERFC_RATIO: log_erfc_and_ratio(x, &r0, &r1); break;
    case PPCX_MATH_CELL: (void)cell_eval<2, false>(y[i], x, x2, gp, s_tab, acc); r0 = acc.SL; r1 = acc.Sq; break;
    case PPCX_MATH_CELL_WIN: (void)cell_eval_win<2, false>(y[i], x, x2, 1.0, gp, s_win, acc); r0 = acc.SL; r1 = acc.Sq; break;
    case PPCX_MATH_CELL_Y: (void)cell_eval<2, false>(y[i], x, x2, gp, s_tab, acc); r0 = acc.SA; r1 = acc.SYq; break;
    case PPCX_MATH_CELL_WIN_Y: (void)cell_eval_win<2, false>(y[i], x, x2, 1.0, gp, s_win, acc); r0 = acc.SA; r1 = acc.SYq; break;
    case PPCX_MATH_SINCOS_2PI: sincos_2pi(x, &r0, &r1); break;
    case PPCX_MATH_LGAMMA_INT1: r0 = lgamma_int1(x); break;
    case PPCX_MATH_RNG_EXP: r0 = rng_exp(x); break;
    case PPCX_MATH_RNG_DIV: r0 = rng_div(x, x2); break;
    case PPCX_MATH_NB2_TAILS: (void)nb2_log_tails(y[i], x, x2, &r0, &r1); break;
    default: r0 = r1 = 0.0; break;
  }
  out0[i] = r0; out1[i] = r1;
}

}  // namespace ppcx

using namespace ppcx;

extern "C" int ppcx_testing_eval_math(int fn, int n, const double* a, const double* b, const int* y, double* out0, double* out1) {
  if (fn < 0 || fn >= PPCX_MATH_COUNT || n < 0 || !a || !b || !y || !out0 || !out1) return PPCX_ERR_ARG;
  if (n == 0) return PPCX_OK;
  std::vector<double> tabs(2 * kLogTabSize + 2 * kWinTabSize);
  fill_log_table(tabs.data());
  fill_window_log_table(tabs.data() + 2 * kLogTabSize);
  const size_t nd = sizeof(double) * (size_t)n;
  double *d_a = nullptr, *d_b = nullptr, *d_tabs = nullptr, *d_o0 = nullptr, *d_o1 = nullptr;
  int* d_y = nullptr;
  int rc = PPCX_OK;
#define TM_CHK(expr) do { if ((expr) != hipSuccess) { rc = PPCX_ERR_HIP; goto done; } } while (0)
  TM_CHK(hipMalloc(&d_a, nd)); TM_CHK(hipMalloc(&d_b, nd)); TM_CHK(hipMalloc(&d_o0, nd)); TM_CHK(hipMalloc(&d_o1, nd));
  TM_CHK(hipMalloc(&d_y, sizeof(int) * (size_t)n)); TM_CHK(hipMalloc(&d_tabs, sizeof(double) * tabs.size()));
  TM_CHK(hipMemcpy(d_a, a, nd, hipMemcpyHostToDevice)); TM_CHK(hipMemcpy(d_b, b, nd, hipMemcpyHostToDevice));
  TM_CHK(hipMemcpy(d_y, y, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  TM_CHK(hipMemcpy(d_tabs, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(ppcx_testing_math_kernel, dim3((n + kMathThreads - 1) / kMathThreads), dim3(kMathThreads), 0, nullptr, fn, n,
                     d_a, d_b, d_y, d_tabs, d_tabs + 2 * kLogTabSize, d_o0, d_o1);
  TM_CHK(hipGetLastError());
  TM_CHK(hipMemcpy(out0, d_o0, nd, hipMemcpyDeviceToHost)); TM_CHK(hipMemcpy(out1, d_o1, nd, hipMemcpyDeviceToHost));
done:
#undef TM_CHK
  (void)hipFree(d_a); (void)hipFree(d_b); (void)hipFree(d_o0); (void)hipFree(d_o1); (void)hipFree(d_y); (void)hipFree(d_tabs);
  return rc;
}
