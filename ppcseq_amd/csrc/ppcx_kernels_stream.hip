// ppcx_kernels_stream.hip -- the streamed log-likelihood kernels: ppcx_loglik_stream_kernel<CM, GEN> (ppcx_loglik.h), the form of the
// log-likelihood workgroup that reads exp(exposure_s), the exposures and the design from global memory -- for models whose
// per-sample constants do not fit LDS (ppcx_model_create_ex). The translation unit holds nothing else: these ten instantiations
// times seven lane counts compile beside those of ppcx_kernels.hip, not after them.
#include "ppcx_loglik.h"

namespace ppcx {

const void* loglik_stream_kernel_ptr(int CM, int gen) {
  const void* f = nullptr;
  PPCX_BY_CM_GEN(ppcx_loglik_stream_kernel, CM, gen, f = (const void*)k_);
  return f;
}

}  // namespace ppcx
