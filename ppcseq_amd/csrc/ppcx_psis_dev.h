// ppcx_psis_dev.h -- the workgroup-parallel pieces of a PSIS tail fit on gfx950, shared by the Pareto-k kernel of ADVI fits
// (ppcx_psis.hip) and the PSIS-LOO kernel (ppcx_loo.hip). The statistic itself is ppcx_psis.h; this header only composes its
// building blocks over a workgroup of kPsisThreads threads:
//   psis_block_sum / psis_block_max   fixed-order reductions (the same bits on every call)
//   psis_select_top                   the M + 1 largest of n values exactly: an MSB-first radix selection on order-preserving
//                                     64-bit keys (eight passes of 8 bits, LDS histograms), the keys above the threshold
//                                     collected, and a bitonic sort in LDS -- the order statistics of a full sort
//   psis_fit_tail                     the m-point profile fit of the M exceedances: one wavefront per grid point, then theta^
//                                     and the mean k = mean_i log1p(-theta^ x_i) before the prior adjustment
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_psis.h"

namespace ppcx {

constexpr int kPsisThreads = 256;
constexpr int kPsisWaves = kPsisThreads / 64;
constexpr int kPsisMaxGrid = 96;              // 30 + floor(sqrt(kPsisMaxSel - 1)) = 93 grid points at most

__device__ __forceinline__ double psis_wave_sum(double v) {
#pragma unroll
  for (int msk = 1; msk < 64; msk <<= 1) v += __shfl_xor(v, msk, 64);
  return v;                                    // the same bits in every lane
}
// sum over the workgroup in a fixed order; every thread gets it. red: kPsisWaves doubles of LDS
__device__ inline double psis_block_sum(double v, double* red) {
  v = psis_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kPsisWaves; ++w) s += red[w];
  return s;
}
// maximum over the workgroup (NaN-free inputs); every thread gets it
__device__ inline double psis_block_max(double v, double* red) {
#pragma unroll
  for (int msk = 1; msk < 64; msk <<= 1) v = fmax(v, __shfl_xor(v, msk, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kPsisWaves; ++w) s = fmax(s, red[w]);
  return s;
}

// ascending bitonic sort of the keys s[0 .. npad) (npad a power of two)
__device__ inline void psis_sort(uint64_t* s, int npad) {
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (npad >> 1); i += kPsisThreads) {
        const int lo = 2 * j * (i / j) + (i % j), hi = lo + j;
        const bool up = (lo & k) == 0;
        const uint64_t a = s[lo], b = s[hi];
        if ((a > b) == up) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
}

struct PsisShared {
  int hist[256];
  double red[kPsisWaves];
  double theta[kPsisMaxGrid], ell[kPsisMaxGrid];
  uint64_t prefix; int want, pos; double theta_hat;
};

// The M + 1 largest of V[0 .. n) (no NaN), ascending, into K[0 .. M] (K[M + 1 .. sel_pad) hold the largest key, for the sort).
// Returns the key of the (M + 1)-th largest value; *want_out = how many copies of it are among the M + 1.
__device__ inline uint64_t psis_select_top(const double* V, long n, int M, uint64_t* K, int sel_pad, PsisShared& sh,
                                           int* want_out) {
  const int tid = threadIdx.x, lane = tid & 63;
  // ---- the (M + 1)-th largest key: eight passes of 8 bits from the top
  uint64_t prefix = 0, mask = 0; int want = M + 1;
  for (int shift = 56; shift >= 0; shift -= 8) {
    sh.hist[tid] = 0;                                  // kPsisThreads == 256 bins
    __syncthreads();
    for (long i0 = 0; i0 < n; i0 += kPsisThreads) {    // wave-uniform trip count
      const long i = i0 + tid;
      bool part = false; int dg = 0;
      if (i < n) {
        const uint64_t k = psis_key(V[i]);
        part = (k & mask) == prefix;
        dg = (int)((k >> shift) & 255);
      }
      const unsigned long long act = __ballot(part);
      if (act) {                                       // one atomic per wavefront where its values share the digit
        const int first = __ffsll((long long)act) - 1;
        const int d0 = __shfl(dg, first, 64);
        if (__all(!part || dg == d0)) { if (lane == first) atomicAdd(&sh.hist[d0], __popcll(act)); }
        else if (part) atomicAdd(&sh.hist[dg], 1);
      }
    }
    __syncthreads();
    if (tid == 0) {
      int cum = 0, b = 255;
      for (; b > 0; --b) { if (cum + sh.hist[b] >= want) break; cum += sh.hist[b]; }
      sh.want = want - cum;
      sh.prefix = prefix | ((uint64_t)b << shift);
    }
    __syncthreads();
    prefix = sh.prefix; want = sh.want; mask |= (uint64_t)255 << shift;
  }
  // ---- the M + 1 largest: the keys above the threshold, then `want` copies of it, sorted
  const int n_gt = M + 1 - want;
  if (tid == 0) sh.pos = 0;
  __syncthreads();
  for (long i = tid; i < n; i += kPsisThreads) {
    const uint64_t k = psis_key(V[i]);
    if (k > prefix) K[atomicAdd(&sh.pos, 1)] = k;
  }
  for (int p = n_gt + tid; p < sel_pad; p += kPsisThreads) K[p] = p <= M ? prefix : ~(uint64_t)0;
  __syncthreads();
  psis_sort(K, sel_pad);
  *want_out = want;
  return prefix;
}

// The profile fit of the ascending exceedances X[0 .. M) (LDS; M >= 5): theta^ and the mean k before the prior adjustment
// (ppcx_psis.h steps 3 and 4). Every thread gets both.
__device__ inline void psis_fit_tail(const double* X, int M, PsisShared& sh, double* theta_hat, double* k_mean) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = psis_grid_size(M);
  const double x_max = X[M - 1], xstar = X[psis_xstar_index(M) - 1];
  for (int j = wave; j < m; j += kPsisWaves) {
    const double th = psis_theta(j + 1, m, x_max, xstar);
    double s = 0.0;
    for (int i = lane; i < M; i += 64) s += log1p(-th * X[i]);
    s = psis_wave_sum(s);
    if (lane == 0) { sh.theta[j] = th; sh.ell[j] = psis_ell(th, s / M, M); }
  }
  __syncthreads();
  if (tid == 0) sh.theta_hat = psis_theta_hat(sh.theta, sh.ell, m);
  __syncthreads();
  const double t = sh.theta_hat;
  double s = 0.0;
  for (int i = tid; i < M; i += kPsisThreads) s += log1p(-t * X[i]);
  s = psis_block_sum(s, sh.red);
  *theta_hat = t;
  *k_mean = s / M;
}

}  // namespace ppcx
