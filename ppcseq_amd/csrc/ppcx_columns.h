// ppcx_columns.h -- the host side that the fit diagnostics and the posterior-predictive driver share (ppcx_summary.hip,
// ppcx_psis.hip, ppcx_loo.hip, ppcx_loo_predict.hip, ppcx_reff.hip, ppcx_ppc_exact.hip, ppcx_ppc.hip and their entry points in
// ppcx_fit_api.hip): the owners -- a device buffer, a pinned host buffer, a stream: what a model, a fit, a run and the scratch
// of a call hold their resources in (ppcx_host.h) --, the column-batch driver and the launch of a kernel with dynamic LDS.
// Every driver built from these synchronises its stream before a buffer goes out of scope (finish() below), also after a
// failed launch: nothing is freed under a running kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "ppcx_kernels.h"

namespace ppcx {

// n elements of T on the current device, freed with the object
template <class T>
struct DeviceBuffer {
  T* p = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, sizeof(T) * n); }
  hipError_t alloc_zeroed(size_t n, hipStream_t st) {                   // allocates; the zero fill is ordered on st
    const hipError_t e = alloc(n);
    return e == hipSuccess ? hipMemsetAsync(p, 0, sizeof(T) * n, st) : e;
  }
  hipError_t upload(const T* host, size_t n, hipStream_t st) {          // allocates; the copy is ordered on st
    const hipError_t e = alloc(n);
    return e == hipSuccess ? hipMemcpyAsync(p, host, sizeof(T) * n, hipMemcpyHostToDevice, st) : e;
  }
  hipError_t download(T* host, size_t n, hipStream_t st) const { return hipMemcpyAsync(host, p, sizeof(T) * n, hipMemcpyDeviceToHost, st); }
};

// n elements of T in pinned host memory, freed with the object
template <class T>
struct PinnedBuffer {
  T* p = nullptr;
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  ~PinnedBuffer() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t n) { return hipHostMalloc(&p, sizeof(T) * n); }
};

// a non-blocking stream of the current device, destroyed with the object. An owner declares it before the buffers that
// work on it: members go in reverse order, the stream after them.
struct DeviceStream {
  hipStream_t s = nullptr;
  DeviceStream() = default;
  DeviceStream(const DeviceStream&) = delete;
  DeviceStream& operator=(const DeviceStream&) = delete;
  ~DeviceStream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// the end of every driver: the stream drained whatever happened before, the first error kept
inline hipError_t finish(hipError_t e, hipStream_t st) {
  const hipError_t es = hipStreamSynchronize(st);
  return e == hipSuccess ? es : e;
}

// columns (or cells) of `rows` doubles per batch under a scratch bound: at least one, at most all of them
inline int column_batch(size_t scratch_bytes, long rows, int n_cols) {
  const int batch = (int)std::max<size_t>(1, scratch_bytes / (sizeof(double) * (size_t)rows));
  return batch < n_cols ? batch : n_cols;
}

// The columns `cols` (host; -1: lp) of draws [rows][D] and lp [rows] (device) in batches of column_batch(scratch_bytes, ..):
// each batch gathered into column-major scratch x [nb][rows] (never a second copy of all the draws), then
// body(x, its column ids (device), nb, its part of the device output [n_cols][fields]) launches the statistic. The output is
// copied to out (host) at the end. Synchronous.
template <class Body>
hipError_t for_column_batches(const double* draws, const double* lp, long rows, int D, int n_cols, const int* cols,
                              size_t scratch_bytes, int fields, double* out, hipStream_t st, Body body) {
  const int batch = column_batch(scratch_bytes, rows, n_cols);
  DeviceBuffer<int> d_cols; DeviceBuffer<double> d_x, d_out;
  hipError_t e = d_cols.upload(cols, (size_t)n_cols, st);
  if (e == hipSuccess) e = d_out.alloc((size_t)fields * n_cols);
  if (e == hipSuccess) e = d_x.alloc((size_t)rows * batch);
  for (int b0 = 0; e == hipSuccess && b0 < n_cols; b0 += batch) {
    const int nb = n_cols - b0 < batch ? n_cols - b0 : batch;
    e = launch_summary_gather_kernel(draws, lp, rows, D, d_cols.p + b0, nb, d_x.p, st);
    if (e == hipSuccess) e = body(d_x.p, d_cols.p + b0, nb, d_out.p + (size_t)b0 * fields);
  }
  if (e == hipSuccess) e = d_out.download(out, (size_t)fields * n_cols, st);
  return finish(e, st);
}

// a kernel with `bytes` of dynamic LDS, the kernel's limit raised above the 64 KB default where that takes it
template <class... Args>
hipError_t launch_dynamic_lds(void (*kernel)(Args...), int n_blocks, int threads, size_t bytes, hipStream_t st, const Args&... a) {
  if (bytes > 64u * 1024u) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(threads), bytes, st, a...);
  return hipGetLastError();
}

}  // namespace ppcx
