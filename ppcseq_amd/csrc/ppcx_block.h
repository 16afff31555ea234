// ppcx_block.h -- the workgroup toolkit of the fit diagnostics on gfx950 (ppcx_summary.hip, ppcx_psis.hip, ppcx_loo.hip,
// ppcx_loo_predict.hip, ppcx_reff.hip, ppcx_ppc_exact.hip): a workgroup of kBlockThreads threads in kBlockWaves wavefronts, its
// reductions and its strided sweeps over a cell's draws (draws_sum, draws_max); and
// the cross-lane reduction of one wavefront, which the posterior-predictive kernels (ppcx_ppc.hip: workgroups of 512) share with
// it. Device code only: the `__host__ __device__` statistic headers
// (ppcx_summary.h, ppcx_psis.h, ppcx_loo.h) never include it, the CPU checks compile without it.
// The reduction order is part of the contract (a column's result is the same bits on every call): an xor butterfly within a
// wavefront, then the wavefronts' values red[0 .. kBlockWaves) in index order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ppcx {

constexpr int kBlockThreads = 256;
constexpr int kBlockWaves = kBlockThreads / 64;

// the smallest power of two >= n (1 for n <= 1)
__host__ __device__ __forceinline__ int pow2_at_least(long n) { int p = 1; while (p < n) p <<= 1; return p; }

// op over the wavefront by the xor butterfly (neighbours, pairs of pairs, ...): the same bits in every lane
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int msk = 1; msk < 64; msk <<= 1) v = op(v, __shfl_xor(v, msk, 64));
  return v;
}
__device__ __forceinline__ double block_wave_sum(double v) { return wave_reduce(v, [](double a, double b) { return a + b; }); }
// sum over the workgroup in a fixed order; every thread gets it. red: kBlockWaves doubles of LDS
__device__ inline double block_sum(double v, double* red) {
  v = block_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kBlockWaves; ++w) s += red[w];
  return s;
}
// maximum over the workgroup (NaN-free inputs); every thread gets it
__device__ inline double block_max(double v, double* red) {
  v = wave_reduce(v, [](double a, double b) { return fmax(a, b); });
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kBlockWaves; ++w) s = fmax(s, red[w]);
  return s;
}
// whether b holds in any thread of the workgroup; every thread gets it (a barrier)
__device__ __forceinline__ bool block_any(bool b) { return __syncthreads_or(b ? 1 : 0) != 0; }
// sum over i = 0 .. n - 1 of f(i), thread t taking i = t, t + kBlockThreads, ...; every thread gets it (fixed order).
// draws_max: their maximum (NaN-free values; -INFINITY for an i that takes no part)
template <class F>
__device__ __forceinline__ double draws_sum(long n, double* red, F f) {
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += kBlockThreads) s += f(i);
  return block_sum(s, red);
}
template <class F>
__device__ __forceinline__ double draws_max(long n, double* red, F f) {
  double m = -INFINITY;
  for (long i = threadIdx.x; i < n; i += kBlockThreads) m = fmax(m, f(i));
  return block_max(m, red);
}

// ascending bitonic sort of s[0 .. npad) (npad a power of two; the caller pads with the largest value): double or uint64_t
template <class T>
__device__ inline void block_sort(T* s, int npad) {
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (npad >> 1); i += kBlockThreads) {
        const int lo = 2 * j * (i / j) + (i % j), hi = lo + j;
        const bool up = (lo & k) == 0;
        const T a = s[lo], b = s[hi];
        if ((a > b) == up) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
}

}  // namespace ppcx
