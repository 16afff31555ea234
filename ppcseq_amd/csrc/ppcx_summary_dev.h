// ppcx_summary_dev.h -- what the kernels that run the split-chain R-hat / Geyer ESS share on the device (ppcx_summary.hip: the fit
// summary per column; ppcx_reff.hip: the relative efficiency per cell): the shared block of a workgroup and the estimator over m
// sequences held in LDS or in the workgroup's slice of global scratch. The statistic is ppcx_summary.h; the workgroup pieces are
// ppcx_block.h.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_block.h"
#include "ppcx_summary.h"
#include "ppcx_kernels.h"

namespace ppcx {

constexpr int kSummaryLags = 16;              // autocovariance lags per chunk (even: a chunk holds whole Geyer pairs)

struct SummaryShared {
  double red[kBlockWaves];
  double rho[kSummaryLags];
  double part[kBlockWaves][kSummaryLags];
  double seq_mean[2 * kSummaryMaxChains];
  double seq_var[2 * kSummaryMaxChains];
};

// R-hat of the m sequences z[j n' .. (j + 1) n'), and with want_ess their ESS (z is then centred in place). One wavefront per
// sequence for the means and variances; the autocovariances summed over all sequences in chunks of kSummaryLags lags.
__device__ inline double summary_sequences(double* z, int m, int nh, bool want_ess, double* ess, SummaryShared& sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < m; j += kBlockWaves) {
    const double* q = z + (long)j * nh;
    double s = 0.0;
    for (int i = lane; i < nh; i += 64) s += q[i];
    const double mu = block_wave_sum(s) / nh;
    double v = 0.0;
    for (int i = lane; i < nh; i += 64) { const double d = q[i] - mu; v += d * d; }
    v = block_wave_sum(v) / (nh - 1.0);
    if (lane == 0) { sh.seq_mean[j] = mu; sh.seq_var[j] = v; }
  }
  __syncthreads();
  double mm = 0.0, mv = 0.0;
  for (int j = 0; j < m; ++j) { mm += sh.seq_mean[j]; mv += sh.seq_var[j]; }
  mm /= m; mv /= m;
  double vm = 0.0;
  for (int j = 0; j < m; ++j) vm += (sh.seq_mean[j] - mm) * (sh.seq_mean[j] - mm);
  vm /= (m - 1.0);
  const double rh = rhat_from(vm, mv, nh);
  if (!want_ess) return rh;
  const double vp = var_plus_of(vm, mv, nh);
  if (!(vp > 0.0)) { *ess = NAN; __syncthreads(); return rh; }
  const long N = (long)m * nh;
  for (long k = threadIdx.x; k < N; k += kBlockThreads) z[k] -= sh.seq_mean[k / nh];
  __syncthreads();
  Geyer g;                                      // every thread runs the same scalar recurrence on the same values
  bool started = false;
  for (int t0 = 0; ; t0 += kSummaryLags) {
    double acc[kSummaryLags];
#pragma unroll
    for (int l = 0; l < kSummaryLags; ++l) acc[l] = 0.0;
    for (long k = threadIdx.x; k < N; k += kBlockThreads) {
      const int i = (int)(k % nh);
      const double c = z[k];
#pragma unroll
      for (int l = 0; l < kSummaryLags; ++l) if (i + t0 + l < nh) acc[l] += c * z[k + t0 + l];
    }
#pragma unroll
    for (int l = 0; l < kSummaryLags; ++l) {
      const double v = block_wave_sum(acc[l]);
      if (lane == 0) sh.part[wave][l] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSummaryLags) {
      double s = 0.0;
      for (int w = 0; w < kBlockWaves; ++w) s += sh.part[w][threadIdx.x];
      sh.rho[threadIdx.x] = rho_of(s / (double)N, mv, vp);
    }
    __syncthreads();
    if (!started) { g.start(nh, sh.rho[1]); started = true; }
    while (g.wants() && g.next() + 1 < t0 + kSummaryLags) { const int t = g.next() - t0; g.feed(sh.rho[t], sh.rho[t + 1]); }
    const bool more = g.wants();
    __syncthreads();                            // rho is rewritten by the next chunk
    if (!more) break;
  }
  *ess = g.ess(N);
  return rh;
}

}  // namespace ppcx
