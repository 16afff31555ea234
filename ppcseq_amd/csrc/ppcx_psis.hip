// ppcx_psis.hip -- gfx950 kernels of the Pareto-k diagnostic of an ADVI fit (ppcx_fit_psis, include/ppcx.h; the statistic:
// ppcx_psis.h).
//
//   ppcx_psis_approx_kernel   the fitted approximation (mu, omega) out of the ADVI state into the fit: the genes' coordinates
//                             from slot 0's vectors, the six hyper-parameters from its hyper vectors.
//   ppcx_psis_stage_kernel    rows of the kept draws into the evaluation slots, as the ADVI kernel writes a Monte-Carlo draw
//                             (V_Q1 and the coordinate constants, the hyper-parameters and an evaluation command per slot); the
//                             log-likelihood / close / reduce kernels the ELBO runs then evaluate them.
//   ppcx_psis_record_kernel   each slot's log density (hyper_close of its reduced sums, as the ELBO kernel forms it) to log_p.
//   ppcx_psis_log_g_kernel    one workgroup per draw: log_g = -1/2 sum_d ((theta_d - mu_d) exp(-omega_d))^2 (Stan's meanfield
//                             calc_log_g) in a fixed order, and r = log_p - log_g (-Inf where either is not finite).
//   ppcx_psis_kernel          one workgroup per column of a batch that ppcx_summary_gather_kernel moved into column-major
//                             scratch (column -1: r): the column's values (1/2 log1p(theta^2) + r), the (M + 1)-th largest of
//                             them by an MSB-first radix selection on order-preserving 64-bit keys (eight passes of 8 bits,
//                             LDS histograms), the M + 1 largest collected and bitonic-sorted in LDS -- exactly the order
//                             statistics of a full sort --, then the m-point profile fit: one wavefront per grid point, a
//                             fixed-order reduction, and theta^ and k-hat as the header composes them. Columns of up to
//                             kPsisLdsDraws draws are staged in LDS, longer ones are transformed in place in the scratch.
// The selection, the sort and the profile fit are in ppcx_psis_dev.h, shared with the PSIS-LOO kernel (ppcx_loo.hip).
// Every reduction runs in a fixed order: a column's k-hat depends on its values only, the same bits on every call.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "ppcx_psis_dev.h"
#include "ppcx_kernels.h"

namespace ppcx {

__global__ __launch_bounds__(256) void ppcx_psis_approx_kernel(Dims d, const double* sq, const double* sg, const double* hyper,
                                                               double* mu, double* omega) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.D) return;
  const int k = i < 3 ? i : (i >= d.off_tail ? 3 + (i - d.off_tail) : -1);
  mu[i] = k < 0 ? sq[i] : hyper[V_SQ * 8 + k];
  omega[i] = k < 0 ? sg[i] : hyper[V_SG * 8 + k];
}

__global__ __launch_bounds__(256) void ppcx_psis_stage_kernel(Dims d, const double* draws, long row0, int n_slots, double* vecs,
                                                              long Dpad, Cmd* cmds) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < d.D; i += gridDim.x * 256) {
    for (int c = 0; c < n_slots; ++c) {
      const double z = draws[(row0 + c) * d.D + i];
      vecs[((long)c * V_COUNT + V_Q1) * Dpad + i] = z;
      coord_consts(d, VecRef{vecs + (long)c * V_COUNT * Dpad, Dpad}, i, z);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < n_slots) {
    const int c = threadIdx.x;
    Cmd& cm = cmds[c];
    for (int k = 0; k < 6; ++k) cm.hyp_q[k] = draws[(row0 + c) * d.D + hyper_index(d, k)];
    cm.type = CMD_EVAL; cm.dir = 1; cm.eps = 0.0; cm.pre_flags = 0; cm.n_merge = 0; cm.subtree_complete = 0; cm.leaf_n = 0;
    cm.hy = make_hyper(cm.hyp_q, d.lambda_mu_mu);
  }
}

__global__ void ppcx_psis_record_kernel(Dims d, const Cmd* cmds, const double* red, int n_slots, double* log_p) {
  const int c = threadIdx.x;
  if (c >= n_slots) return;
  const Cmd& cm = cmds[c];
  const double* r = red + (long)c * PT_COUNT;
  double g6[6];
  log_p[c] = hyper_close(d, cm.hy, cm.hyp_q, r[PT_LP], r + PT_H0, g6);
}

__global__ __launch_bounds__(kPsisThreads) void ppcx_psis_log_g_kernel(const double* draws, int D, const double* mu,
                                                                       const double* omega, const double* log_p, double* log_g,
                                                                       double* r) {
  __shared__ double red[kPsisWaves];
  const long row = blockIdx.x;
  const double* x = draws + row * D;
  double s = 0.0;
  for (int i = threadIdx.x; i < D; i += kPsisThreads) {
    const double z = (x[i] - mu[i]) * exp(-omega[i]);
    s += z * z;
  }
  const double lg = -0.5 * psis_block_sum(s, red);
  if (threadIdx.x == 0) {
    const double lp = log_p[row];
    log_g[row] = lg;
    r[row] = isfinite(lp) && isfinite(lg) ? lp - lg : -INFINITY;
  }
}

template <bool LDS>
__global__ __launch_bounds__(kPsisThreads) void ppcx_psis_kernel(PsisArgs a) {
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  const int tid = threadIdx.x;
  const long n = a.n;
  uint64_t* K = lds_u;                                   // [sel_pad] keys of the M + 1 largest values
  double* X = reinterpret_cast<double*>(lds_u + a.sel_pad);            // [sel_pad] the tail's exceedances
  for (int c = blockIdx.x; c < a.n_cols; c += gridDim.x) {
    const int col = a.cols[c];
    double* V = LDS ? X + a.sel_pad : a.x + (long)c * n;  // the column's values
    // ---- the values, their count N (the -Inf entries take no part), a NaN / +Inf entry
    bool bad = false; double cnt = 0.0;
    for (long i = tid; i < n; i += kPsisThreads) {
      const double v = psis_value(a.x[(long)c * n + i], a.r[i], col);
      bad = bad || isnan(v) || v == INFINITY;
      cnt += v != -INFINITY ? 1.0 : 0.0;
      V[i] = v;
    }
    bad = __syncthreads_or(bad ? 1 : 0) != 0;
    const long N = (long)psis_block_sum(cnt, sh.red);
    const int M = psis_tail_len(N);
    if (bad || M < 5 || (long)M >= N) {
      if (tid == 0) a.out[c] = bad ? NAN : INFINITY;
      __syncthreads();
      continue;
    }
    int want;
    (void)psis_select_top(V, n, M, K, a.sel_pad, sh, &want);
    const double cut = psis_unkey(K[0]), mx = psis_unkey(K[M]);
    if (psis_unkey(K[1]) == mx) {                        // the M tail values are all equal
      if (tid == 0) a.out[c] = INFINITY;
      __syncthreads();
      continue;
    }
    const double ec = exp(cut - mx);
    for (int i = tid; i < M; i += kPsisThreads) X[i] = exp(psis_unkey(K[i + 1]) - mx) - ec;
    __syncthreads();
    // ---- the profile fit: one wavefront per grid point
    double theta_hat, k_mean;
    psis_fit_tail(X, M, sh, &theta_hat, &k_mean);
    if (tid == 0) a.out[c] = psis_adjust(k_mean, M);
    __syncthreads();                                     // K, X, V and the shared block are reused by the next column
  }
}

// ---- launch helpers (host)
static int psis_pow2(long n) { int p = 1; while (p < n) p <<= 1; return p; }
int psis_sel_pad(long n) { return psis_pow2((long)psis_tail_len(n) + 1); }
hipError_t launch_psis_approx_kernel(const Dims& d, const double* sq, const double* sg, const double* hyper, double* mu, double* omega,
                                     hipStream_t st) {
  hipLaunchKernelGGL(ppcx_psis_approx_kernel, dim3((unsigned)((d.D + 255) / 256)), dim3(256), 0, st, d, sq, sg, hyper, mu, omega);
  return hipGetLastError();
}
hipError_t launch_psis_stage_kernel(const Dims& d, const double* draws, long row0, int n_slots, double* vecs, long Dpad, Cmd* cmds,
                                    hipStream_t st) {
  int nb = (d.D + 255) / 256; if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(ppcx_psis_stage_kernel, dim3(nb), dim3(256), 0, st, d, draws, row0, n_slots, vecs, Dpad, cmds);
  return hipGetLastError();
}
hipError_t launch_psis_record_kernel(const Dims& d, const Cmd* cmds, const double* red, int n_slots, double* log_p, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_psis_record_kernel, dim3(1), dim3(256), 0, st, d, cmds, red, n_slots, log_p);
  return hipGetLastError();
}
hipError_t launch_psis_log_g_kernel(const double* draws, long rows, int D, const double* mu, const double* omega, const double* log_p,
                                    double* log_g, double* r, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_psis_log_g_kernel, dim3((unsigned)rows), dim3(kPsisThreads), 0, st, draws, D, mu, omega, log_p, log_g, r);
  return hipGetLastError();
}
hipError_t launch_psis_kernel(const PsisArgs& a, hipStream_t st) {
  const bool lds = a.n <= kPsisLdsDraws;
  const size_t bytes = sizeof(double) * (2 * (size_t)a.sel_pad + (lds ? (size_t)a.n : 0));
  const void* fn = lds ? (const void*)ppcx_psis_kernel<true> : (const void*)ppcx_psis_kernel<false>;
  if (bytes > 64u * 1024u) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  if (lds) hipLaunchKernelGGL(ppcx_psis_kernel<true>, dim3(a.n_cols), dim3(kPsisThreads), bytes, st, a);
  else hipLaunchKernelGGL(ppcx_psis_kernel<false>, dim3(a.n_cols), dim3(kPsisThreads), bytes, st, a);
  return hipGetLastError();
}

// k-hat of the columns `cols` (host array; -1: r) of the draws [n][D] (device), r [n] (device): the columns go through
// column-major scratch in batches of at most scratch_bytes (never a second copy of all the draws). Synchronous.
hipError_t psis_columns(const double* draws, const double* r, long n, int D, int n_cols, const int* cols, double* khat,
                        size_t scratch_bytes, hipStream_t st) {
  int batch = (int)std::max<size_t>(1, scratch_bytes / (sizeof(double) * (size_t)n));
  if (batch > n_cols) batch = n_cols;
  int* d_cols = nullptr; double *d_x = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_cols, sizeof(int) * (size_t)n_cols);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * (size_t)n_cols);
  if (e == hipSuccess) e = hipMalloc(&d_x, sizeof(double) * (size_t)n * batch);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cols, cols, sizeof(int) * (size_t)n_cols, hipMemcpyHostToDevice, st);
  for (int b0 = 0; e == hipSuccess && b0 < n_cols; b0 += batch) {
    const int nb = n_cols - b0 < batch ? n_cols - b0 : batch;
    e = launch_summary_gather_kernel(draws, r, n, D, d_cols + b0, nb, d_x, st);
    if (e != hipSuccess) break;
    PsisArgs a;
    a.x = d_x; a.r = r; a.cols = d_cols + b0; a.n_cols = nb; a.n = n; a.sel_pad = psis_sel_pad(n); a.out = d_out + b0;
    e = launch_psis_kernel(a, st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(khat, d_out, sizeof(double) * (size_t)n_cols, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);    // also after a failed launch: nothing is freed under a running kernel
  if (e == hipSuccess) e = es;
  (void)hipFree(d_cols); (void)hipFree(d_x); (void)hipFree(d_out);
  return e;
}

}  // namespace ppcx
