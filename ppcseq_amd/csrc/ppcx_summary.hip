// ppcx_summary.hip -- gfx950 kernels of the fit summary (ppcx_fit_summary, include/ppcx.h): per column of the kept draws the
// plain summary, the rank-normalised split R-hat and the bulk / tail ESS (the statistics: ppcx_summary.h).
//
//   ppcx_summary_gather_kernel  a batch of columns of the draws [M n][D] (or lp__) into column-major scratch [batch][M n],
//                               32 x 33 LDS tiles: reads along the columns, writes along the draws, both coalesced.
//   ppcx_summary_kernel<LDS>    one workgroup per column: bitonic sort of the split values, average ranks by binary search of
//                               the sorted copy (exact for ties, no index array), Blom z, the sequences' means and variances
//                               (one wavefront per sequence), the autocovariances in chunks of kSummaryLags lags as far as
//                               Geyer's truncation asks for them. LDS = true: the sort buffer and the sequence values live in
//                               LDS (columns of up to kSummaryLdsDraws draws); LDS = false: the same code on a slice of a
//                               global scratch buffer per workgroup (longer columns; a workgroup's own stores are visible to
//                               its waves after the barrier, as in the posterior-predictive kernel's global path).
// A column's result depends on its draws only (fixed reduction orders): the same bits on every call and in both paths.
#include <hip/hip_runtime.h>
#include "ppcx_summary_dev.h"
#include "ppcx_columns.h"

namespace ppcx {

__global__ __launch_bounds__(256) void ppcx_summary_gather_kernel(const double* draws, const double* lp, long rows, int D,
                                                                  const int* cols, int n_cols, double* out) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
  const long r0 = (long)blockIdx.x * 32; const int c0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const long row = r0 + r; const int c = c0 + tx;
    double v = 0.0;
    if (row < rows && c < n_cols) { const int col = cols[c]; v = col < 0 ? lp[row] : draws[row * D + col]; }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r; const long row = r0 + tx;
    if (row < rows && c < n_cols) out[(long)c * rows + row] = tile[tx][r];
  }
}

template <bool LDS>
__global__ __launch_bounds__(kBlockThreads) void ppcx_summary_kernel(SummaryArgs a) {
  extern __shared__ double lds[];
  __shared__ SummaryShared sh;
  const long Mn = (long)a.M * a.n;
  const int nh = a.n / 2, m = 2 * a.M;
  const long N = (long)m * nh;
  double* S = LDS ? lds : a.scratch + (long)blockIdx.x * a.slice;     // [npad] the sort buffer
  double* Z = S + a.npad;                                              // [N] the sequences
  for (int c = blockIdx.x; c < a.n_cols; c += gridDim.x) {
    const double* x = a.x + (long)c * Mn;
    double* out = a.out + (long)c * SUM_FIELDS;
    // ---- plain summary over all M n draws
    double s = 0.0; bool bad = false;
    for (long i = threadIdx.x; i < Mn; i += kBlockThreads) { const double v = x[i]; bad = bad || !isfinite(v); s += v; }
    bad = block_any(bad);
    const double mean = block_sum(s, sh.red) / (double)Mn;
    if (bad) {
      if (threadIdx.x < SUM_FIELDS) out[threadIdx.x] = NAN;
      continue;
    }
    double ss = 0.0;
    for (long i = threadIdx.x; i < Mn; i += kBlockThreads) { const double d = x[i] - mean; ss += d * d; }
    ss = block_sum(ss, sh.red);
    double q05 = 0.0, q50 = 0.0, q95 = 0.0;
    if (N != Mn || nh < 2) {                    // odd n (the split values drop the middle draws) or nothing to split
      const int np = pow2_at_least(Mn);
      for (long i = threadIdx.x; i < np; i += kBlockThreads) S[i] = i < Mn ? x[i] : INFINITY;
      __syncthreads();
      block_sort(S, np);
      q05 = quantile7_sorted(S, Mn, 0.05); q50 = quantile7_sorted(S, Mn, 0.5); q95 = quantile7_sorted(S, Mn, 0.95);
      __syncthreads();
    }
    double rhat = NAN, ess_bulk = NAN, ess_tail = NAN;
    if (nh >= 2) {
      const int np = pow2_at_least(N);
      for (long k = threadIdx.x; k < np; k += kBlockThreads) S[k] = k < N ? x[split_source(k, nh, a.n)] : INFINITY;
      __syncthreads();
      block_sort(S, np);
      const double sq05 = quantile7_sorted(S, N, 0.05), med = quantile7_sorted(S, N, 0.5), sq95 = quantile7_sorted(S, N, 0.95);
      if (N == Mn) { q05 = sq05; q50 = med; q95 = sq95; }
      if (S[0] < S[N - 1]) {
        for (long k = threadIdx.x; k < N; k += kBlockThreads) Z[k] = blom_z(average_rank(S, N, x[split_source(k, nh, a.n)]), N);
        __syncthreads();
        const double rb = summary_sequences(Z, m, nh, true, &ess_bulk, sh);
        __syncthreads();                        // S and Z are rewritten below
        for (long k = threadIdx.x; k < np; k += kBlockThreads) S[k] = k < N ? fabs(x[split_source(k, nh, a.n)] - med) : INFINITY;
        __syncthreads();
        block_sort(S, np);
        for (long k = threadIdx.x; k < N; k += kBlockThreads) Z[k] = blom_z(average_rank(S, N, fabs(x[split_source(k, nh, a.n)] - med)), N);
        __syncthreads();
        const double rf = summary_sequences(Z, m, nh, false, nullptr, sh);
        rhat = fmax(rb, rf);
        __syncthreads();
        double e05 = NAN, e95 = NAN;
        for (long k = threadIdx.x; k < N; k += kBlockThreads) Z[k] = x[split_source(k, nh, a.n)] <= sq05 ? 1.0 : 0.0;
        __syncthreads();
        summary_sequences(Z, m, nh, true, &e05, sh);
        __syncthreads();
        for (long k = threadIdx.x; k < N; k += kBlockThreads) Z[k] = x[split_source(k, nh, a.n)] <= sq95 ? 1.0 : 0.0;
        __syncthreads();
        summary_sequences(Z, m, nh, true, &e95, sh);
        ess_tail = isnan(e05) ? e95 : (isnan(e95) ? e05 : (e05 < e95 ? e05 : e95));
      }
    }
    if (threadIdx.x == 0) {
      out[SUM_MEAN] = mean; out[SUM_SD] = sqrt(ss / ((double)Mn - 1.0));
      out[SUM_Q05] = q05; out[SUM_Q50] = q50; out[SUM_Q95] = q95;
      out[SUM_RHAT] = rhat; out[SUM_ESS_BULK] = ess_bulk; out[SUM_ESS_TAIL] = ess_tail;
    }
    __syncthreads();                            // S, Z and the shared block are reused by the next column
  }
}

// ---- launch helpers (host)
int summary_npad(int M, int n) { return pow2_at_least((long)M * n); }
long summary_slice_doubles(int M, int n) { return (long)summary_npad(M, n) + 2L * M * (n / 2) + 1; }
size_t summary_lds_bytes(int M, int n) { return (long)M * n <= kSummaryLdsDraws ? sizeof(double) * (size_t)summary_slice_doubles(M, n) : 0; }
hipError_t launch_summary_gather_kernel(const double* draws, const double* lp, long rows, int D, const int* cols, int n_cols, double* out, hipStream_t st) {
  const dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((n_cols + 31) / 32));
  hipLaunchKernelGGL(ppcx_summary_gather_kernel, grid, dim3(256), 0, st, draws, lp, rows, D, cols, n_cols, out);
  return hipGetLastError();
}
hipError_t launch_summary_kernel(const SummaryArgs& a, int nblocks, hipStream_t st) {
  if (a.scratch) return launch_dynamic_lds(ppcx_summary_kernel<false>, nblocks, kBlockThreads, 0, st, a);
  return launch_dynamic_lds(ppcx_summary_kernel<true>, nblocks, kBlockThreads, summary_lds_bytes(a.M, a.n), st, a);
}

// The summary of the columns `cols` (host; -1: lp) of M chains of n draws [M n][D] (device) into out [n_cols][SUM_FIELDS] (host).
// Half of scratch_bytes bounds a batch's columns ([batch][M n]), the other half the global path's slices, one per workgroup
// (at most 2048 of them). Synchronous.
hipError_t summary_columns(const double* draws, const double* lp, int M, int n, int D, int n_cols, const int* cols, double* out,
                           size_t scratch_bytes, hipStream_t st) {
  const long rows = (long)M * n;
  const bool lds = summary_lds_bytes(M, n) > 0;
  const long slice = summary_slice_doubles(M, n);
  int nslices = lds ? 0 : column_batch(scratch_bytes / 2, slice, column_batch(scratch_bytes / 2, rows, n_cols));
  if (nslices > 2048) nslices = 2048;
  DeviceBuffer<double> d_scr;
  hipError_t e = lds ? hipSuccess : d_scr.alloc((size_t)slice * nslices);
  if (e != hipSuccess) return e;
  return for_column_batches(draws, lp, rows, D, n_cols, cols, scratch_bytes / 2, SUM_FIELDS, out, st,
                            [&](const double* x, const int*, int nb, double* d_out) {
    SummaryArgs a;
    a.x = x; a.n_cols = nb; a.M = M; a.n = n; a.npad = summary_npad(M, n);
    a.out = d_out; a.scratch = d_scr.p; a.slice = slice;
    return launch_summary_kernel(a, lds ? nb : nslices, st);
  });
}

}  // namespace ppcx
