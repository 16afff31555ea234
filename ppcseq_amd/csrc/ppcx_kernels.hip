// ppcx_kernels.hip -- the LDS-staged log-likelihood kernels: ppcx_loglik_kernel<CM, GEN> (ppcx_loglik.h), instantiated through its
// launch helpers, and the host helpers that the merged launch (ppcx_kernels_ls.hip) shares with them. The other kernel families
// of the engine have translation units of their own (the index: ppcx_kernels.h).
#include <hip/hip_runtime.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"
#include "ppcx_loglik.h"

namespace ppcx {

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
int loglik_generic_possible(const Dims& d) { return !d.x0_is_one ? 2 : ((d.C >= 2 && d.K > 0 && !d.x1_binary) ? 1 : 0); }
// LDS of a log-likelihood workgroup: the two tables, exp(exposure_s), and the design columns its genes read -- columns 1 .. C - 1
// where X[,1] == 1 (sweep_cells: S * C doubles in all; 8 960 samples fit at C = 2), the exposures and the whole of X for a design
// without the column of ones (generic_cells: S * (2 + C))
// streamed (ppcx_model_create_ex): the tables only -- the sweep reads the per-sample constants from global memory
size_t loglik_lds_bytes(const Dims& d, bool streamed) {
  if (streamed) return sizeof(double) * (2 * kLogTabSize + 2 * kWinTabSize);
  const size_t per_sample = loglik_generic_possible(d) == 2 ? (size_t)(2 + d.C) : (size_t)(d.C < 1 ? 1 : d.C);
  return sizeof(double) * (2 * kLogTabSize + 2 * kWinTabSize + (size_t)d.S * per_sample + 2 * kLdsPad);
}
static const void* loglik_kernel_ptr(int CM, int gen, bool streamed) {
  if (streamed) return loglik_stream_kernel_ptr(CM, gen);
  const void* f = nullptr;
  PPCX_BY_CM_GEN(ppcx_loglik_kernel, CM, gen, f = (const void*)k_);
  return f;
}
// workgroups of 256 threads of kernel f that a CU holds with lds_bytes of dynamic LDS each (0: the query failed)
int resident_workgroups_per_cu(const void* f, size_t lds_bytes) {
  if (lds_bytes > 64u * 1024u) {               // more than the default limit of dynamic LDS: ask for it once
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  }
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 256, lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}
int loglik_resident_workgroups_per_cu(int CM, const Dims& d, bool streamed) {
  return resident_workgroups_per_cu(loglik_kernel_ptr(CM, loglik_generic_possible(d), streamed), loglik_lds_bytes(d, streamed));
}
hipError_t launch_loglik_kernel(int CM, const LoglikArgs& a, bool streamed, hipStream_t st) {
  const size_t lds_bytes = loglik_lds_bytes(a.d, streamed);
  const dim3 grid((unsigned)((a.nbpc + 7) / 8 * 8) * (unsigned)a.nchains);
  LoglikArgs args = a;
  void* params[] = {&args};
  return hipLaunchKernel(loglik_kernel_ptr(CM, loglik_generic_possible(a.d), streamed), grid, dim3(256), params, lds_bytes, st);
}

}  // namespace ppcx
