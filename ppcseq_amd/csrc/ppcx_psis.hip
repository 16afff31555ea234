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
#include "ppcx_columns.h"

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

__global__ __launch_bounds__(kBlockThreads) void ppcx_psis_log_g_kernel(const double* draws, int D, const double* mu,
                                                                       const double* omega, const double* log_p, double* log_g,
                                                                       double* r) {
  __shared__ double red[kBlockWaves];
  const long row = blockIdx.x;
  const double* x = draws + row * D;
  double s = 0.0;
  for (int i = threadIdx.x; i < D; i += kBlockThreads) {
    const double z = (x[i] - mu[i]) * exp(-omega[i]);
    s += z * z;
  }
  const double lg = -0.5 * block_sum(s, red);
  if (threadIdx.x == 0) {
    const double lp = log_p[row];
    log_g[row] = lg;
    r[row] = isfinite(lp) && isfinite(lg) ? lp - lg : -INFINITY;
  }
}

template <bool LDS>
__global__ __launch_bounds__(kBlockThreads) void ppcx_psis_kernel(PsisArgs a) {
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
    for (long i = tid; i < n; i += kBlockThreads) {
      const double v = psis_value(a.x[(long)c * n + i], a.r[i], col);
      bad = bad || isnan(v) || v == INFINITY;
      cnt += v != -INFINITY ? 1.0 : 0.0;
      V[i] = v;
    }
    bad = block_any(bad);
    const long N = (long)block_sum(cnt, sh.red);
    // ---- the tail: the M + 1 largest, the profile fit (one wavefront per grid point), k-hat
    const int M = psis_tail_len(N);
    PsisTail t;
    const PsisTailStatus ts = bad ? PSIS_TAIL_SHORT : psis_tail(V, n, N, M, K, X, a.sel_pad, sh, &t);
    if (tid == 0) a.out[c] = bad ? NAN : (ts == PSIS_TAIL_FITTED ? psis_adjust(t.k_mean, M) : INFINITY);
    __syncthreads();                                     // K, X, V and the shared block are reused by the next column
  }
}

// ---- launch helpers (host)
int psis_sel_pad(long n) { return pow2_at_least((long)psis_tail_len(n) + 1); }
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
  hipLaunchKernelGGL(ppcx_psis_log_g_kernel, dim3((unsigned)rows), dim3(kBlockThreads), 0, st, draws, D, mu, omega, log_p, log_g, r);
  return hipGetLastError();
}
hipError_t launch_psis_kernel(const PsisArgs& a, hipStream_t st) {
  const bool lds = a.n <= kPsisLdsDraws;
  const size_t bytes = sizeof(double) * (2 * (size_t)a.sel_pad + (lds ? (size_t)a.n : 0));
  return launch_dynamic_lds(lds ? ppcx_psis_kernel<true> : ppcx_psis_kernel<false>, a.n_cols, kBlockThreads, bytes, st, a);
}

// k-hat of the columns `cols` (host array; -1: r) of the draws [n][D] (device), r [n] (device): the columns go through
// column-major scratch in batches of at most scratch_bytes (never a second copy of all the draws). Synchronous.
hipError_t psis_columns(const double* draws, const double* r, long n, int D, int n_cols, const int* cols, double* khat,
                        size_t scratch_bytes, hipStream_t st) {
  return for_column_batches(draws, r, n, D, n_cols, cols, scratch_bytes, 1, khat, st,
                            [&](double* x, const int* d_cols, int nb, double* d_out) {
    PsisArgs a;
    a.x = x; a.r = r; a.cols = d_cols; a.n_cols = nb; a.n = n; a.sel_pad = psis_sel_pad(n); a.out = d_out;
    return launch_psis_kernel(a, st);
  });
}

}  // namespace ppcx
