// ppcx_kernels_close.hip -- the per-gene close in both round structures: ppcx_close_kernel<CM> of the three-launch round and
// ppcx_gene_kernel<CM> of a pipelined round (what they compute per gene: ppcx_gene.h), the wavefront and workgroup sums that
// feed the slab, and their launch helpers.
#include <hip/hip_runtime.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"

namespace ppcx {


// -----------------------------------------------------------------------------------------------------
// kernel A2: one thread per gene closes it -- priors, gradient, second half kick of the gene's coordinates,
// U-turn dot products and subtree slots -- and the workgroup leaves its partial sums in a slab.
// -----------------------------------------------------------------------------------------------------
// sum over the wavefront, left in lane 63: inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4, 8), then the
// row totals travel to the next row (row_bcast:15 into rows 1 and 3) and to the upper half (row_bcast:31 into rows 2, 3)
__device__ __forceinline__ double wave_sum_to_lane63(double v) {
  v += dpp_take<0x111, 0xf>(v);
  v += dpp_take<0x112, 0xf>(v);
  v += dpp_take<0x114, 0xf>(v);
  v += dpp_take<0x118, 0xf>(v);
  v += dpp_take<0x142, 0xa>(v);
  v += dpp_take<0x143, 0xc>(v);
  return v;
}
template <int N>
__device__ __forceinline__ void block_accumulate(double* vals, double* wacc, int wave, int lane) {
#pragma unroll
  for (int k = 0; k < N; ++k) vals[k] = wave_sum_to_lane63(vals[k]);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < N; ++k) wacc[wave * PT_COUNT + k] = vals[k];
  }
}
// leaf_close's reducer of the close kernel: every group of six by the cross-lane scan
struct ScanSums {
  static constexpr bool kLevel0WithLeaf = false;
  double* wacc; int wave, lane;
  __device__ __forceinline__ double* begin(int, double* own) {
#pragma unroll
    for (int k = 0; k < 6; ++k) own[k] = 0.0;
    return own;
  }
  __device__ __forceinline__ void end(int off, double* six) { block_accumulate<6>(six, wacc + off, wave, lane); }
};
// after a workgroup barrier: the four wavefronts' partial sums -> the workgroup's row of the slab, zeros where the command
// produced nothing. keep_t0: column PT_T0 was left by the round that applied the command (gene kernel) and stays
__device__ __forceinline__ void slab_row_write(const Cmd& c, const double* wacc, double* slab, int tid, bool keep_t0) {
  const int np = parts_used(c);
  for (int k = tid; k < np; k += 256) {
    if (keep_t0 && k == PT_T0) continue;
    const bool used = k < 10 || (k >= PT_DOTS && k < PT_DOTS + 6 * c.n_merge) || (k >= PT_TOP && c.subtree_complete);
    slab[k] = used ? ((wacc[k] + wacc[PT_COUNT + k]) + wacc[2 * PT_COUNT + k]) + wacc[3 * PT_COUNT + k] : 0.0;
  }
}

// Sums of up to 16 quantities over the 64 lanes of a wavefront THROUGH LDS: row k = quantity k, one column per lane, rows padded
// to 65 doubles; lane 4 k + part adds columns 16 part .. 16 part + 15 of row k, the four parts meet by two cross-lane
// moves, and the lanes 4 k .. 4 k + 3 end with the total of quantity k. About 25 vector instructions and 32 LDS accesses for 16 sums,
// against 18 vector instructions PER sum of the cross-lane scan (wave_sum_to_lane63): the gene kernel spent a quarter of its 1100
// vector instructions per wavefront in those scans (profiles/r04_sq_counters_gene.txt). Fixed order, the scan's own (below): the same bits as before.
constexpr int kRowStride = 65, kPartStride = 16, kRowsPerWave = 16;     // 39 808 bytes of LDS per gene workgroup: four per CU (below)
template <int N>
__device__ __forceinline__ void wave_sums_lds(const double* vals, double* rows, double* out /* wacc + offset */, int lane) {
  static_assert(N >= 1 && N <= kRowsPerWave, "one batch");
#pragma unroll
  for (int k = 0; k < N; ++k) rows[k * kRowStride + lane + (kPartStride - 16) * (lane >> 4)] = vals[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int k = lane >> 2, part = lane & 3;
  double t = 0.0;
  if (k < N) {
    // the sixteen columns in the order of the cross-lane scan this replaces (wave_sum_to_lane63: neighbours, pairs of pairs,
    // ... -- a balanced tree), so that the sums, and with them every fit, keep the bits they had
    const double* r = rows + k * kRowStride + kPartStride * part;
    double b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = r[2 * j + 1] + r[2 * j];
    t = ((b[7] + b[6]) + (b[5] + b[4])) + ((b[3] + b[2]) + (b[1] + b[0]));
  }
  t += dpp_take<0xB1, 0xf>(t);                 // quad_perm [1,0,3,2]: parts 0 + 1, 2 + 3
  t += dpp_take<0x4E, 0xf>(t);                 // quad_perm [2,3,0,1]: the quad's total
  if (k < N && part == 0) out[k] = t;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();             // the rows are free again
}

template <int CM>
__global__ __launch_bounds__(256) void ppcx_close_kernel(CloseArgs a) {
  constexpr int NCM = CM + 1;
  constexpr int NS = GeneSums<CM>::N;
  __shared__ double wacc[4 * PT_COUNT];
  const int chain = blockIdx.y;
  const Cmd& c = a.cmds[chain];
  if (c.type == CMD_DONE || c.type == CMD_FLUSH) return;
  const Dims& d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const VecRef v{a.vecs + (long)chain * V_COUNT * a.Dpad, a.Dpad};
  const double* sums = a.sums + (long)chain * NS * d.G;
  const int g = blockIdx.x * 256 + tid;
  GeneCtx<CM> x;
  gene_load<CM>(d, c, v, g, x);
  GeneSumsV<CM> acc;
  gene_sums_load<CM>(d, sums, g, x.active, acc);
  SlotPre<CM, 3> pre;                          // requested now, behind the gene's arithmetic
  slot_prefetch<CM, 3>(c, v, x, true, pre);
  double pn[NCM], minv[NCM], part[10];
  gene_finish<CM>(d, c, v, x, acc, a.Sy, a.SyE, a.SyX, a.SX, a.ncell, a.Lg1, part, pn, minv);
  block_accumulate<10>(part, wacc, wave, lane);
  if (c.type == CMD_LEAF) {
    ScanSums r{wacc, wave, lane};
    leaf_close<CM, 3>(c, v, x, pn, minv, pre, r);
  }
  __syncthreads();
  slab_row_write(c, wacc, a.partials + ((long)chain * gridDim.x + blockIdx.x) * PT_COUNT, tid, false);
}

// leaf_close's reducer of the gene kernel: sums through LDS. The ten sums of the leaf travel with the six U-turn products of the
// first level it closes, one batch of 16: part[0 .. 9] the leaf, part[10 .. 15] level 0, which lands in
// wrow[PT_DOTS .. PT_DOTS + 5]; every other group in a batch of its own.
struct LdsSums {
  static constexpr bool kLevel0WithLeaf = true;
  static_assert(PT_DOTS == 10, "the first level's products follow the leaf's ten sums");
  double* part; double* rows; double* wrow; int lane;
  __device__ __forceinline__ double* begin(int off, double* own) {
    double* six = off == PT_DOTS ? part + 10 : own;
#pragma unroll
    for (int k = 0; k < 6; ++k) six[k] = 0.0;
    return six;
  }
  __device__ __forceinline__ void end(int off, double* six) {
    if (off == PT_DOTS) wave_sums_lds<16>(part, rows, wrow, lane);
    else wave_sums_lds<6>(six, rows, wrow + off, lane);
  }
};

// One gene's part of a pipelined round, for the lane that owns gene g (g >= G: a lane without a gene, which only takes part
// in the reductions): the command's work on the gene's coordinates, the close of the evaluated position, the anticipated
// constants. No workgroup barrier inside; the wavefront's partial sums go to wacc[wave][...]. Everything the lane reads is
// requested in one burst at the start: nothing else hides this kernel's latency.
// (Kept apart from the kernel's barriers because a fused one-launch round was built on it in round 3 -- the wavefront that
// swept a range of genes closed them itself after its chain's state machine, a workgroup of the same launch, had published the
// command through a flag -- and measured: 90 us per launch against 63 + 20 for the two launches)
template <int CM>
__device__ __forceinline__ void gene_wave_part(const GeneArgs& ga, const Cmd& c, int chain, int g,
                                               double* wacc, double* rows, int wave, int lane, bool do_update, bool do_close) {
  constexpr int NCM = CM + 1;
  constexpr int NS = GeneSums<CM>::N;
  const CloseArgs& a = ga.c;
  const Dims& d = a.d;
  const VecRef v{a.vecs + (long)chain * V_COUNT * a.Dpad, a.Dpad};
  const double* sums = a.sums + (long)chain * NS * d.G;
  GeneCtx<CM> x;
  gene_index<CM>(d, g, x);
  // ---- a command with rare pre-operations: those first, through memory (gene_rare_pre)
  double T0 = 0.0;
  double* draws = ga.draws ? ga.draws + (long)chain * ga.draws_chain_stride : nullptr;
  const int fmask = do_update ? gene_rare_pre<CM>(d, c, v, x, draws, &T0) : ~0;
  // ---- everything this lane reads is requested here, in one round trip, before anything is stored
  CoordCache cache[NCM];
  double p_cur[NCM], minv[NCM];
#pragma unroll
  for (int j = 0; j < NCM; ++j) {
    p_cur[j] = 0.0; minv[j] = 1.0; x.q[j] = 0.0;
    if (j < x.ncoord) {
      if (do_update) cache[j] = coord_prefetch_for(c, v, x.idx[j]);
      else { x.q[j] = v.at(V_Q0 + 3 * c.dir, x.idx[j]); p_cur[j] = v.at(V_P0 + 3 * c.dir, x.idx[j]); minv[j] = v.at(V_MINV, x.idx[j]); }
    }
  }
  GeneSumsV<CM> acc;
  GeneData gd;
  double phi = 1.0;
  constexpr int kPreLev = 2;                   // tree levels whose slots travel with the burst of loads (a third: 18 registers; see the kernel)
  SlotPre<CM, kPreLev> pre;
  gene_sums_load<CM>(d, sums, g, do_close && x.active, acc);
  if (do_close) {
    // phi of the position being closed: written with the constants the log-likelihood part evaluated (for a leaf
    // anticipated by the previous round the update below does not touch them)
    if (x.active) phi = v.at(V_C0, x.idx[1]);
    gene_data_load<CM>(d, x.gg, a.Sy, a.SyE, a.SyX, a.SX, a.ncell, a.Lg1, gd);
  }
  slot_prefetch<CM, kPreLev>(c, v, x, do_close, pre);
  // ---- the command's work on the gene's coordinates
  if (do_update) gene_coord_update<CM, true>(d, c, v, x, draws, &T0, !do_close, cache, p_cur, minv, !do_close, fmask);
  if (!do_close) {                             // the command's position has not been evaluated yet: nothing to close
    double t0v[1] = {T0};
    wave_sums_lds<1>(t0v, rows, wacc + wave * PT_COUNT, lane);
    return;
  }
  // ---- close the evaluated position
  x.gp.coef[0] = x.q[0];
#pragma unroll
  for (int cc = 1; cc < CM; ++cc) x.gp.coef[cc] = (x.has_slopes && cc < d.C) ? x.q[cc + 1] : 0.0;
  x.gp.sigma_raw = x.q[1];
  x.gp.phi = phi; x.gp.invphi = 0.0;
  double pn[NCM], gn[NCM], part[16];
  gene_finish_vals<CM>(d, c, v, x, acc, gd, p_cur, minv, part, pn, gn);
  part[PT_T0] = T0;
  double* wrow = wacc + wave * PT_COUNT;
  if (c.type != CMD_LEAF) { wave_sums_lds<10>(part, rows, wrow, lane); return; }
  LdsSums r{part, rows, wrow, lane};
  leaf_close<CM, kPreLev>(c, v, x, pn, minv, pre, r);
  // ahead of the state machine: the constants of the position the next leaf evaluates if the tree goes on
  if (ga.spec) gene_spec_consts<CM>(d, c, v, x, pn, gn, minv);
}
// after a workgroup barrier: the four wavefronts' partial sums -> the workgroup's row of the slab
__device__ __forceinline__ void gene_block_finish(const Cmd& c, bool do_update, bool do_close, const double* wacc, double* slab, int tid) {
  if (!do_close) {
    if (tid == 0) slab[PT_T0] = ((wacc[0] + wacc[PT_COUNT]) + wacc[2 * PT_COUNT]) + wacc[3 * PT_COUNT];
    return;
  }
  slab_row_write(c, wacc, slab, tid, !do_update);
}

// Register budget of the two-column instantiation: 128 vector registers, four wavefronts per SIMD -- what a log-likelihood
// wavefront holds. In a fit with chain groups this kernel starts while another group's log-likelihood wavefronts, four to a SIMD,
// own every register of the chip: a wavefront of 128 registers moves in as soon as ONE of them retires, a wavefront of 146 (152
// allocated: what the body took with three prefetched tree levels) only after two on the same SIMD have, and this kernel is what
// its group's next log-likelihood launch waits for. cfg3, 8 chains in three groups (round 4, five seeds, alternating builds):
// 2.52 s per fit with 146 registers, 2.41 s with 128 and 36 of them spilled, 2.35 s with two prefetched levels instead of three
// (kPreLev: 128 registers without a spill; alone on the chip as fast as before, 2.94 s on one stream, 1.03 s a lone chain).
// (Four columns: 230 registers; 168 or 128 with 120 / 202 spilled made the factor design's fits 7 % / 14 % slower.)
template <int CM>
__global__ __launch_bounds__(256, CM <= 2 ? 4 : (CM <= 4 ? 2 : 1)) void ppcx_gene_kernel(GeneArgs ga) {
  __shared__ double wacc[4 * PT_COUNT];
  __shared__ double s_rows[4 * kRowsPerWave * kRowStride];      // wave_sums_lds: 8.3 KB per wavefront
  const CloseArgs& a = ga.c;
  const int chain = blockIdx.y;
  // the chain's command, copied into registers HERE: read through the reference its fields would be requested where they are
  // first used -- after the barrier below, a scalar round trip in front of the loads whose addresses depend on them
  const Cmd c = a.cmds[chain];
  if (c.type == CMD_DONE) return;
  const bool do_update = !c.updated, do_close = c.evaluated && c.type != CMD_FLUSH;      // uniform over the launch's chain
  if (!do_update && !do_close) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  gene_wave_part<CM>(ga, c, chain, blockIdx.x * 256 + tid, wacc, s_rows + wave * kRowsPerWave * kRowStride, wave, lane, do_update, do_close);
  __syncthreads();
  gene_block_finish(c, do_update, do_close, wacc, a.partials + ((long)chain * gridDim.x + blockIdx.x) * PT_COUNT, tid);
}

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
// the instantiation of a kernel that has one per number of design columns only
#define PPCX_BY_CM(KERNEL, CM) \
  ((CM) <= 2 ? (const void*)KERNEL<2> : (CM) <= 4 ? (const void*)KERNEL<4> : (CM) <= 8 ? (const void*)KERNEL<8> : (const void*)KERNEL<16>)
hipError_t launch_close_kernel(int CM, const CloseArgs& a, int nblocks, int nchains, hipStream_t st) {
  CloseArgs args = a;
  void* params[] = {&args};
  return hipLaunchKernel(PPCX_BY_CM(ppcx_close_kernel, CM), dim3(nblocks, nchains), dim3(256), params, 0, st);
}
hipError_t launch_gene_kernel(int CM, const GeneArgs& a, int nblocks, int nchains, hipStream_t st) {
  GeneArgs args = a;
  void* params[] = {&args};
  return hipLaunchKernel(PPCX_BY_CM(ppcx_gene_kernel, CM), dim3(nblocks, nchains), dim3(256), params, 0, st);
}

}  // namespace ppcx
