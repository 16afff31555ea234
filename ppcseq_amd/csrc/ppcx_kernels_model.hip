// ppcx_kernels_model.hip -- what a model and its retained draws need outside a round: ppcx_disp_build_kernel (the genes'
// dispersion tables, ppcx_disp.h), ppcx_gather_kernel (column gather of the draws) and ppcx_fill_kernel, with their launch
// helpers.
#include <hip/hip_runtime.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"

namespace ppcx {

// -----------------------------------------------------------------------------------------------------
// The genes' dispersion tables (ppcx_disp.h), built once per model and whenever the exclusions change: one workgroup per
// gene. Phase 1: thread (panel, node) evaluates Fh and Dh at its node -- a loop over the gene's row in LDS, every thread on
// the same cell (so the y < 8 / y >= 8 branch of disp_cell is uniform). Phase 2: thread (panel, function) turns the panel's
// node values into its polynomial. 352 nodes x S cells per gene: a few milliseconds at 20 000 x 200.
// -----------------------------------------------------------------------------------------------------
constexpr int kDispThreads = 384;             // 352 nodes: one round
__global__ __launch_bounds__(kDispThreads) void ppcx_disp_build_kernel(const int* counts, int G, int S, const int* genes, int n_genes,
                                                                        DispFit fit, double* table) {
  extern __shared__ int s_row[];              // S counts, then (8-byte aligned) 2 x kDispPanels x kDispN node values
  const int gi = blockIdx.x;
  if (gi >= n_genes) return;
  const int g = genes ? genes[gi] : gi;
  const int tid = threadIdx.x;
  double* s_val = reinterpret_cast<double*>(s_row + ((S + 1) & ~1));
  for (int s = tid; s < S; s += kDispThreads) s_row[s] = counts[(long)g * S + s];
  __syncthreads();
  constexpr int NN = kDispPanels * kDispN;
  for (int t = tid; t < NN; t += kDispThreads) {
    const int p = t / kDispN, k = t - p * kDispN;
    double lo;
    const double sg = disp_node_sigma(fit, p, k, &lo);
    const DispPoint pt = disp_point(sg, lo);
    double F, D;
    disp_row(s_row, S, 0, 1, pt, &F, &D);
    s_val[(p * 2 + 0) * kDispN + k] = F; s_val[(p * 2 + 1) * kDispN + k] = D;
  }
  __syncthreads();
  for (int t = tid; t < 2 * kDispPanels; t += kDispThreads) {
    double out[kDispStride];
    disp_fit_panel(fit, s_val + t * kDispN, out);
    double* dst = table + (long)g * kDispGeneDoubles + (long)t * kDispStride;
#pragma unroll
    for (int m = 0; m < kDispStride; ++m) dst[m] = out[m];
  }
}

__global__ void ppcx_gather_kernel(const double* draws, long n_rows, int D, const int* cols, int n_cols, double* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows * n_cols) return;
  const long r = i / n_cols; const int cidx = (int)(i % n_cols);
  out[i] = draws[r * D + cols[cidx]];
}

__global__ void ppcx_fill_kernel(double* p, long n, double val) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = val;
}

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
size_t disp_build_lds_bytes(int S) { return sizeof(int) * (size_t)((S + 1) & ~1) + sizeof(double) * 2 * kDispPanels * kDispN; }
hipError_t launch_disp_build_kernel(const int* counts, int G, int S, const int* genes, int n_genes, const DispFit& fit, double* table, hipStream_t st) {
  const size_t lds = disp_build_lds_bytes(S);
  if (lds > 64u * 1024u) {
    hipError_t e = hipFuncSetAttribute((const void*)ppcx_disp_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ppcx_disp_build_kernel, dim3((unsigned)n_genes), dim3(kDispThreads), lds, st, counts, G, S, genes, n_genes, fit, table);
  return hipGetLastError();
}
hipError_t launch_gather_kernel(const double* draws, long n_rows, int D, const int* cols, int n_cols, double* out, hipStream_t st) {
  const long n = n_rows * n_cols;
  hipLaunchKernelGGL(ppcx_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, draws, n_rows, D, cols, n_cols, out);
  return hipGetLastError();
}
hipError_t launch_fill_kernel(double* p, long n, double val, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, val);
  return hipGetLastError();
}

}  // namespace ppcx
