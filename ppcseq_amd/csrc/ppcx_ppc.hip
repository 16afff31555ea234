// ppcx_ppc.hip -- gfx950 kernels of the posterior-predictive draws and their credible intervals (generated quantities,
// .stan:259-266, and rstan::summary's mean / sd / two quantiles; ppcx_fit_ppc, include/ppcx.h; the statistic: ppcx_ppc.h), and
// their driver ppc_fit at the end of this file.
//
//   ppcx_ppc_table_kernel  the checked genes' parameters, transposed: T[g][c][draw] with phi in the last row (ppcx_table.h).
//   ppcx_ppc_wave_kernel   ONE WAVEFRONT per (gene < K, sample) cell, up to kPpcWaveMaxDraws predictive draws per cell. The lanes'
//                          rejection samplers run in ONE loop of attempts (cell_draws); mean, sd and the order statistics around
//                          the two type-7 quantiles are taken inside the wavefront (cross-lane moves, no workgroup barrier).
//   ppcx_ppc_kernel        one workgroup of kPpcThreads per cell for longer ones: the cell's draws in LDS up to kPpcLdsDraws,
//                          beyond that in the workgroup's slice of a global scratch, the workgroups taking cells in turn.
// Both kernels end in the same summary (cell_summary) over their own reductions (WaveCell, BlockCell), whose orders are part
// of the contract: a cell's four fields are the same bits on every call.
#include <hip/hip_runtime.h>
#include "ppcx_block.h"
#include "ppcx_columns.h"
#include "ppcx_table.h"

namespace ppcx {

constexpr int kPpcThreads = 512;              // 8 wavefronts share the cell's draws in LDS (2 per SIMD: up to 256 VGPRs, the kernel needs ~200)
constexpr int kPpcWaves = kPpcThreads / 64;
// draws of a cell that ppcx_ppc_kernel keeps in LDS: a CU has 160 KB, the kernel's static LDS (BlockCell's sred and s_cnt, 4128
// bytes) gets 5 KB of it, the integers the other 155 KB
constexpr int kPpcLdsDraws = 39680;
constexpr int kPpcWaveMaxDraws = 4096;        // per cell: 16 KB of integers per wavefront, 64 KB per workgroup, two workgroups per CU
// integers between the cells of the four wavefronts of a ppcx_ppc_wave_kernel workgroup: n_gen rounded up to an even number
__host__ __device__ constexpr int ppc_wave_stride(int n_gen) { return (n_gen + 1) & ~1; }
static_assert(sizeof(int) * kPpcLdsDraws + sizeof(double) * kPpcThreads + sizeof(int) * kPpcWaves <= 160 * 1024, "LDS of a CU");

__global__ __launch_bounds__(256) void ppcx_ppc_table_kernel(const double* draws, long n_draws, Dims d, double tc, double* T) {
  table_tiles<true>(draws, n_draws, d, nullptr, d.K, tc, T);
}

// cell = g S + s, which is also its Philox address (ppc_cell_address): its sample, its gene's rows of T, its exposure
struct PpcCell { int cell, s; const double* Tg; double expo; };
__device__ __forceinline__ PpcCell ppc_cell(const PpcArgs& a, const double* T, int cell) {
  const int g = cell / a.d.S, s = cell - g * a.d.S;
  return PpcCell{cell, s, T + (long)g * (a.d.C + 1) * a.n_draws, a.exposure[s]};
}
// eta and phi of the cell's predictive draw j
__device__ __forceinline__ void ppc_draw_params(const PpcArgs& a, const PpcCell& c, int j, double* eta, double* phi) {
  const long src = a.resample ? ppc_resample_src((uint32_t)j, (uint32_t)c.cell, a.k0, a.n_draws) : j;
  table_draw(c.Tg, a.n_draws, a.d.C, c.expo, a.X, a.d.S, c.s, src, eta, phi);
}
// draw j of the cell is val: into the cell's array, its running sum and maximum, and the caller's matrix where it asked for one
__device__ __forceinline__ void ppc_keep(const PpcArgs& a, int cell, int j, int val, int* vals, double* sum, int* vmax) {
  vals[j] = val;
  *sum += (double)val; *vmax = val > *vmax ? val : *vmax;
  if (a.counts_rng) a.counts_rng[(long)j * a.n_cells + cell] = val;
}

// The predictive draws of one cell by `stride` cooperating lanes (lane `first` takes draws first, first + stride, ...):
// ONE loop of attempts for the wavefront. Per turn a lane makes one attempt at the gamma variate of its current draw (or begins
// the draw) and, once it has it, one attempt at the Poisson variate (gamma_attempt / poisson_attempt, ppcx_math.h); a lane whose
// draw is complete stores it and begins its next draw in the next turn. A draw costs a lane ~1.15 turns (the two samplers'
// rejection rates) instead of every draw waiting for the slowest lane's rejections.
__device__ __forceinline__ void cell_draws(const PpcArgs& a, const double* T, int cell, int* vals, int first, int stride,
                                           double* sum_out, int* vmax_out) {
  const int n = a.n_gen;
  const PpcCell c = ppc_cell(a, T, cell);
  double sum = 0.0; int vmax = 0;
  int j = first, phase = 0;                     // 0: begin the draw, 1: gamma attempts, 2: Poisson attempts
  GammaDraw gd; PoissonDraw pq; double scale = 0.0;
  while (PPCX_WAVE_ANY(j < n)) {
    if (j < n) {
      int val = 0; bool done = false;
      if (phase == 0) {                         // the draw's parameters, the gamma stream
        double eta, phi;
        ppc_draw_params(a, c, j, &eta, &phi);
        if (nb2_invalid(eta, phi)) { val = kPpcInvalid; done = true; }
        else { gamma_begin(gd, phi, a.k0, (uint32_t)cell, (uint32_t)j); scale = rng_div(rng_exp(eta), phi); phase = 1; }
      }
      if (phase == 1) {
        double gam;
        if (gamma_attempt(gd, &gam)) {
          const double lam = gam * scale;
          if (!(lam < 1073741824.0)) { val = kPpcSaturated; done = true; }
          else { poisson_begin(pq, lam, a.k0, (uint32_t)cell, (uint32_t)j); phase = 2; }
        }
      }
      if (phase == 2 && !done) {
        long long k;
        if (poisson_attempt(pq, &k)) { val = k > 2147483647LL ? 2147483647 : (int)k; done = true; }
      }
      if (done) {
        ppc_keep(a, cell, j, val, vals, &sum, &vmax);
        j += stride; phase = 0;
      }
    }
  }
  *sum_out = sum; *vmax_out = vmax;
}

// The lanes that share a cell -- `first` is this lane among them, it holds draws first, first + kStride, ... -- and their
// reductions, every lane getting the result. A wavefront: the xor butterfly.
struct WaveCell {
  static constexpr int kStride = 64;
  int first;
  template <class Op> __device__ __forceinline__ int reduce(int v, Op op) const { return wave_reduce(v, op); }
  __device__ __forceinline__ double sum(double v) const { return block_wave_sum(v); }
};
// The workgroup of kPpcThreads: integers by the butterfly, then the wavefronts' values s_cnt[0 .. kPpcWaves) in index order;
// a sum of doubles by the tree over sred[0 .. kPpcThreads). Two barriers each.
struct BlockCell {
  static constexpr int kStride = kPpcThreads;
  int first;
  double* sred; int* s_cnt;
  template <class Op> __device__ __forceinline__ int reduce(int v, Op op) const {
    v = wave_reduce(v, op);
    if ((first & 63) == 0) s_cnt[first >> 6] = v;
    __syncthreads();
    int tot = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kPpcWaves; ++w) tot = op(tot, s_cnt[w]);
    __syncthreads();
    return tot;
  }
  __device__ __forceinline__ double sum(double v) const {
    sred[first] = v;
    __syncthreads();
    for (int st = kPpcThreads / 2; st > 0; st >>= 1) { if (first < st) sred[first] += sred[first + st]; __syncthreads(); }
    const double tot = sred[0];
    __syncthreads();
    return tot;
  }
};

// mean, sd and the two type-7 quantiles of the cell's draws vals[0 .. n) into ci[cell]; sum and vmax: this lane's share
template <class Lanes>
__device__ __forceinline__ void cell_summary(const PpcArgs& a, int cell, const Lanes& l, const int* vals, double sum, int vmax) {
  const int n = a.n_gen;
  const double mean = l.sum(sum) / (double)n;
  double ss = 0.0;
  for (int j = l.first; j < n; j += Lanes::kStride) { const double t = (double)vals[j] - mean; ss += t * t; }
  const double sd = n > 1 ? sqrt(l.sum(ss) / (double)(n - 1)) : NAN;
  vmax = l.reduce(vmax, [](int x, int y) { return y > x ? y : x; });     // upper end of the bisections
  auto count_le = [&](int v) {
    int c = 0;
    for (int j = l.first; j < n; j += Lanes::kStride) c += vals[j] <= v ? 1 : 0;
    return l.reduce(c, [](int x, int y) { return x + y; });
  };
  auto min_above = [&](int v) {
    int mn = 2147483647;
    for (int j = l.first; j < n; j += Lanes::kStride) { const int x = vals[j]; mn = (x > v && x < mn) ? x : mn; }
    return l.reduce(mn, [](int x, int y) { return y < x ? y : x; });
  };
  double q[2];
  const double pr[2] = {a.p_lo, a.p_hi};
  for (int k = 0; k < 2; ++k) {
    double h; long lo; int v0, v1;
    type7_rank(n, pr[k], &h, &lo);
    select_pair(n, (int)lo, vmax, count_le, min_above, &v0, &v1);
    q[k] = type7(h, lo, n, (double)v0, (double)v1);
  }
  if (l.first == 0) {
    double* o = a.ci + (long)cell * 4;
    o[0] = mean; o[1] = sd; o[2] = q[0]; o[3] = q[1];
  }
}

__global__ __launch_bounds__(kPpcThreads) void ppcx_ppc_kernel(PpcArgs a, const double* T) {
  extern __shared__ int ldsi[];
  __shared__ double sred[kPpcThreads];
  __shared__ int s_cnt[kPpcWaves];
  const int tid = threadIdx.x;
  // a cell's draws live in LDS when they fit (one workgroup per cell), otherwise in this workgroup's slice of a global
  // scratch buffer, and the workgroup takes cells in turn (how_many_posterior_draws = draws_after_tail / threshold
  // reaches 100 000 at the reference's defaults with 200 samples, R/methods.R:166-167)
  int* vals = a.scratch ? a.scratch + (long)blockIdx.x * a.n_gen : ldsi;
  const int n = a.n_gen;
  for (int cell = blockIdx.x; cell < a.n_cells; cell += gridDim.x) {
    // eight wavefronts share the cell here: every lane has few draws, and draw after draw (each wavefront waiting for its
    // slowest lane) measured faster than the one loop of attempts that the wavefront-per-cell kernel runs (145 vs 185 ms at
    // 10 500 draws per cell x 200 000 cells)
    const PpcCell c = ppc_cell(a, T, cell);
    double sum = 0.0; int vmax = 0;
    for (int j = tid; j < n; j += kPpcThreads) {
      double eta, phi;
      ppc_draw_params(a, c, j, &eta, &phi);
      ppc_keep(a, cell, j, nb2_log_rng(eta, phi, a.k0, (uint32_t)cell, (uint32_t)j), vals, &sum, &vmax);
    }
    cell_summary(a, cell, BlockCell{tid, sred, s_cnt}, vals, sum, vmax);
    __syncthreads();                             // the next cell reuses vals
  }
}

__global__ __launch_bounds__(256) void ppcx_ppc_wave_kernel(PpcArgs a, const double* T) {
  extern __shared__ int ldsw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int* vals = ldsw + (long)wave * ppc_wave_stride(a.n_gen);                   // [n_gen] the cell's draws
  for (int cell = blockIdx.x * 4 + wave; cell < a.n_cells; cell += gridDim.x * 4) {
    double sum = 0.0; int vmax = 0;
    cell_draws(a, T, cell, vals, lane, 64, &sum, &vmax);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the lanes' integers are in LDS before any lane reads another's
    __builtin_amdgcn_wave_barrier();
    cell_summary(a, cell, WaveCell{lane}, vals, sum, vmax);
    __builtin_amdgcn_wave_barrier();             // the next cell reuses vals
  }
}

// The driver of ppcx_fit_ppc. Of `a` the caller gives the model, the draws, the probabilities, the seed and n_gen (device
// pointers); ci [n_cells][4] and counts_rng [n_gen][n_cells] (or null) are host. kernel_ms: the table and the kernel by HIP events
// (left alone where there are none). Synchronous.
hipError_t ppc_fit(PpcArgs a, double* ci, int32_t* counts_rng, float* kernel_ms, hipStream_t st) {
  // one wavefront per cell, four cells per workgroup; beyond kPpcWaveMaxDraws one workgroup per cell; beyond kPpcLdsDraws
  // 1024 workgroups share the cells and keep the current cell's draws in their slice of a global scratch buffer
  const bool wave = a.n_gen <= kPpcWaveMaxDraws, lds = a.n_gen <= kPpcLdsDraws;
  const int n_blocks = wave ? std::min((a.n_cells + 3) / 4, 4096) : lds ? a.n_cells : std::min(a.n_cells, 1024);
  const size_t bytes = sizeof(int) * (wave ? 4 * (size_t)ppc_wave_stride(a.n_gen) : lds ? (size_t)a.n_gen : 0);
  DeviceBuffer<double> d_ci, d_T;                // d_T: the checked genes' parameters, transposed: [K][C + 1][draws]
  DeviceBuffer<int> d_rng, d_scratch;
  hipError_t e = d_ci.alloc((size_t)a.n_cells * 4);
  if (e == hipSuccess) e = d_T.alloc((size_t)a.d.K * (a.d.C + 1) * (size_t)a.n_draws);
  if (e == hipSuccess && !lds) e = d_scratch.alloc((size_t)n_blocks * a.n_gen);
  if (e == hipSuccess && counts_rng) e = d_rng.alloc((size_t)a.n_gen * a.n_cells);
  if (e != hipSuccess) return e;
  a.ci = d_ci.p; a.counts_rng = d_rng.p; a.scratch = d_scratch.p;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  (void)hipEventCreate(&ev0); (void)hipEventCreate(&ev1);
  if (ev0) (void)hipEventRecord(ev0, st);
  hipLaunchKernelGGL(ppcx_ppc_table_kernel, dim3((unsigned)((a.n_draws + 31) / 32), (unsigned)((a.d.K + 31) / 32)), dim3(256), 0, st,
                     a.draws, a.n_draws, a.d, a.truncation_compensation, d_T.p);
  e = hipGetLastError();
  if (e == hipSuccess) e = launch_dynamic_lds(wave ? ppcx_ppc_wave_kernel : ppcx_ppc_kernel, n_blocks, wave ? 256 : kPpcThreads, bytes, st,
                                              a, (const double*)d_T.p);
  if (ev1) (void)hipEventRecord(ev1, st);
  if (e == hipSuccess) e = d_ci.download(ci, (size_t)a.n_cells * 4, st);
  if (e == hipSuccess && counts_rng) e = d_rng.download(counts_rng, (size_t)a.n_gen * a.n_cells, st);
  e = finish(e, st);                             // drained whatever happened: the buffers go out of scope below
  float ms = 0;
  if (e == hipSuccess && ev0 && ev1 && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) *kernel_ms = ms;
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  return e;
}

}  // namespace ppcx
