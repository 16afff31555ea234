// ppcx_psis_dev.h -- the workgroup-parallel pieces of a PSIS tail fit on gfx950, shared by the Pareto-k kernel of ADVI fits
// (ppcx_psis.hip) and the PSIS-LOO kernel (ppcx_loo.hip). The statistic itself is ppcx_psis.h; this header only composes its
// building blocks over a workgroup of kBlockThreads threads (ppcx_block.h: the fixed-order reductions and the bitonic sort):
//   psis_select_top                   the M + 1 largest of n values exactly: an MSB-first radix selection on order-preserving
//                                     64-bit keys (eight passes of 8 bits, LDS histograms), the keys above the threshold
//                                     collected, and a bitonic sort in LDS -- the order statistics of a full sort
//   psis_fit_tail                     the m-point profile fit of the M exceedances: one wavefront per grid point, then theta^
//                                     and the mean k = mean_i log1p(-theta^ x_i) before the prior adjustment
//   psis_tail                         the two in a row, from a column's values to its fitted tail
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_block.h"
#include "ppcx_psis.h"

namespace ppcx {

constexpr int kPsisMaxGrid = 96;              // 30 + floor(sqrt(kPsisMaxSel - 1)) = 93 grid points at most

struct PsisShared {
  int hist[256];
  double red[kBlockWaves];
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
    sh.hist[tid] = 0;                                  // kBlockThreads == 256 bins
    __syncthreads();
    for (long i0 = 0; i0 < n; i0 += kBlockThreads) {    // wave-uniform trip count
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
  for (long i = tid; i < n; i += kBlockThreads) {
    const uint64_t k = psis_key(V[i]);
    if (k > prefix) K[atomicAdd(&sh.pos, 1)] = k;
  }
  for (int p = n_gt + tid; p < sel_pad; p += kBlockThreads) K[p] = p <= M ? prefix : ~(uint64_t)0;
  __syncthreads();
  block_sort(K, sel_pad);
  *want_out = want;
  return prefix;
}

// The profile fit of the ascending exceedances X[0 .. M) (LDS; M >= 5): theta^ and the mean k before the prior adjustment
// (ppcx_psis.h steps 3 and 4). Every thread gets both.
__device__ inline void psis_fit_tail(const double* X, int M, PsisShared& sh, double* theta_hat, double* k_mean) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = psis_grid_size(M);
  const double x_max = X[M - 1], xstar = X[psis_xstar_index(M) - 1];
  for (int j = wave; j < m; j += kBlockWaves) {
    const double th = psis_theta(j + 1, m, x_max, xstar);
    double s = 0.0;
    for (int i = lane; i < M; i += 64) s += log1p(-th * X[i]);
    s = block_wave_sum(s);
    if (lane == 0) { sh.theta[j] = th; sh.ell[j] = psis_ell(th, s / M, M); }
  }
  __syncthreads();
  if (tid == 0) sh.theta_hat = psis_theta_hat(sh.theta, sh.ell, m);
  __syncthreads();
  const double t = sh.theta_hat;
  double s = 0.0;
  for (int i = tid; i < M; i += kBlockThreads) s += log1p(-t * X[i]);
  s = block_sum(s, sh.red);
  *theta_hat = t;
  *k_mean = s / M;
}

// The fitted tail of the values V[0 .. n) (no NaN), M of them in the tail (ppcx_psis.h steps 1 to 3). Every thread gets the same.
enum PsisTailStatus : int { PSIS_TAIL_SHORT = 0, PSIS_TAIL_EQUAL, PSIS_TAIL_FITTED };
struct PsisTail {
  double cut, mx, ec;           // the (M + 1)-th largest value, the largest, exp(cut - mx)           (EQUAL: cut and mx only)
  double theta_hat, k_mean;     // the profile fit: theta^, and the mean k before the prior adjustment
  uint64_t key; int want;       // the key of cut, and how many copies of it are among the M + 1 largest       (also EQUAL)
};
// SHORT: M < 5 or M >= N (the N values that are not -Inf), nothing is touched. EQUAL: the M tail values are all equal, K is
// filled. FITTED: K[0 .. M] hold the keys of the M + 1 largest, ascending, and X[0 .. M) the exceedances exp(v - mx) - ec.
__device__ inline PsisTailStatus psis_tail(const double* V, long n, long N, int M, uint64_t* K, double* X, int sel_pad,
                                           PsisShared& sh, PsisTail* t) {
  if (M < 5 || (long)M >= N) return PSIS_TAIL_SHORT;
  t->key = psis_select_top(V, n, M, K, sel_pad, sh, &t->want);
  t->cut = psis_unkey(K[0]); t->mx = psis_unkey(K[M]);
  if (psis_unkey(K[1]) == t->mx) return PSIS_TAIL_EQUAL;
  t->ec = exp(t->cut - t->mx);
  for (int i = threadIdx.x; i < M; i += kBlockThreads) X[i] = exp(psis_unkey(K[i + 1]) - t->mx) - t->ec;
  __syncthreads();
  psis_fit_tail(X, M, sh, &t->theta_hat, &t->k_mean);
  return PSIS_TAIL_FITTED;
}

}  // namespace ppcx
