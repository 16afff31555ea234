// ppcx_loglik.h -- the log-likelihood workgroup (device): the L-lane reduction, a wavefront's passes over its range of genes, the
// workgroup's body, and the kernel in its two forms -- the per-sample constants staged in LDS (ppcx_kernels.hip) or read from
// global memory (STREAM; ppcx_kernels_stream.hip, a translation unit of its own so that the two sets of instantiations compile
// side by side). ppcx_ls_kernel (ppcx_kernels_ls.hip) runs the same workgroup beside the chains' state machines (ppcx_step.h).
// word_t and dpp_take, which the state machine and the close kernels use as well: ppcx_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"

namespace ppcx {

// 16-byte requests of arrays of doubles (LDS fills)
typedef double2 __attribute__((may_alias)) dpair_t;

// -----------------------------------------------------------------------------------------------------
// kernel A1: the log-likelihood kernel. Streams the count matrix once and leaves, per gene, the sums of
// GeneSumsV (ppcx_model.h): the likelihood part of the gene's log density, its d/dphi part, sum rho
// (+ sum X_sc rho for genes with slopes).
// -----------------------------------------------------------------------------------------------------
#ifndef PPCX_LOGLIK_OCC
#define PPCX_LOGLIK_OCC 2
#endif
#ifndef PPCX_LOGLIK_OCC_FAST
#define PPCX_LOGLIK_OCC_FAST 4                   // wavefronts per SIMD of the instantiation without the per-cell-eta path
#endif
__device__ __forceinline__ double wave_xor_add_rt(double v, int lane_xor_mask) {      // run-time mask: ds_bpermute
  const int src = (int)((threadIdx.x ^ (unsigned)lane_xor_mask) & 63u) << 2;
  const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(v));
  return v + __hiloint2double(hi, lo);
}
// sum over the L lanes that share a gene, every lane ending with the total: inside a row of 16 lanes by DPP moves (neighbours,
// pairs, the other quad by row_half_mirror, the other half-row by row_mirror -- vector-unit moves, no LDS round trips: nine
// dependent ds_bpermute round trips per pass were half a microsecond of nothing but latency), across rows by ds_bpermute
template <int L>
__device__ __forceinline__ double group_sum(double v) {
  if (L >= 2) v += dpp_take<0xB1, 0xf>(v);     // quad_perm [1,0,3,2]
  if (L >= 4) v += dpp_take<0x4E, 0xf>(v);     // quad_perm [2,3,0,1]
  if (L >= 8) v += dpp_take<0x141, 0xf>(v);    // row_half_mirror
  if (L >= 16) v += dpp_take<0x140, 0xf>(v);   // row_mirror
  if (L >= 32) v = wave_xor_add_rt(v, 16);
  if (L >= 64) v = wave_xor_add_rt(v, 32);
  return v;
}
// A resident launch (host: plan_launch): as many workgroups as the chip holds at once (4 per CU at 128 VGPRs), divided
// among the chains; every wavefront owns a contiguous range of the host's gene order -- bounds[j] .. bounds[j + 1] --
// chosen on the host so that all ranges cost the same, and walks it 64 / L genes at a time. All wavefronts start
// together and finish together: no partly filled last round of workgroups, one LDS fill per resident workgroup.
// Wavefronts are independent after the LDS fill (no barrier, no atomic), and a gene's sums depend on L only.
template <int CM, int LG, int GEN, bool STREAM = false>
__device__ __forceinline__ void loglik_passes(const LoglikArgs& a, const Cmd& c, const VecRef& v, double* sums, int p0, int p1,
                                              const double* stab, const double* swin, const double* sE, const double* sExpo, const double* sX,
                                              int lane, bool any_generic) {
  constexpr int L = 1 << LG, GPW = 64 >> LG;     // lanes per gene, genes per wavefront and pass
  const Dims& d = a.d;
  const int sub = lane & (L - 1), gl = lane >> LG;
  // the gene order's base as a value of its own: read out of the kernel's arguments where it is used, it is kept, spilled and
  // brought back in every pass together with the fifteen other words of the argument block it arrived in
  const PPCX_GLOBAL int* order = as_global(a.order);
  asm volatile("" : "+s"(order));
  // One pass ahead: while pass p is swept, the constants of pass p + 1's genes (gene_pre_load) and the gene indices of pass
  // p + 2 are on their way.
  int g_cur = ld32(order, p0 + gl < p1 ? p0 + gl : p1 - 1);
  int g_next = ld32(order, p0 + GPW + gl < p1 ? p0 + GPW + gl : p1 - 1);
  GenePre pre_cur = gene_pre_load(d, v, a.cd, g_cur);
#ifdef PPCX_TRACE
  unsigned long long* tr = nullptr;
  if (a.trace && lane == 0 && (blockIdx.x % 16) == 0 && blockIdx.x / 16 < kTraceBlocks)
    tr = a.trace + (((long)(blockIdx.x / 16) * 4 + (threadIdx.x >> 6)) * kTracePasses) * kTraceStamps;
  int tpass = 0;
#define PPCX_STAMP(k) do { if (tr && tpass < kTracePasses) tr[tpass * kTraceStamps + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define PPCX_STAMP(k) ((void)0)
#endif
  for (int p = p0; p < p1; p += GPW) {
    PPCX_STAMP(0);
#ifdef PPCX_TRACE
    if (tr && tpass < kTracePasses) tr[tpass * kTraceStamps + 7] = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef PPCX_PRIO_BALANCE
    // the SIMD serves its oldest wavefront first, so its four wavefronts (one from each quarter of the launch's workgroups)
    // finish one after the other and the last ones run alone, at a fraction of the issue rate: a wavefront with more passes
    // left goes first instead
    {
      const int rem = (p1 - p + GPW - 1) / GPW;
      if (rem >= 4) __builtin_amdgcn_s_setprio(3); else if (rem == 3) __builtin_amdgcn_s_setprio(2); else if (rem == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
    }
#endif
    const bool act = p + gl < p1;                // lanes past the end of the range repeat its last gene and store nothing
    const int g = g_cur;
    const GenePre pre = pre_cur;
    if (p + GPW < p1) {
      g_cur = g_next;
      pre_cur = gene_pre_load(d, v, a.cd, g_next);
      const int pn = p + 2 * GPW + gl;
      g_next = ld32(order, pn < p1 ? pn : p1 - 1);
    }
    if (CM > 2 && d.x0_is_one && !PPCX_WAVE_ANY(g < d.K)) {
      // a pass of plain genes in a model with more than two design columns: the two-column instantiation of the gene's work
      // (its accumulators carry two slope sums, not CM: the registers the wider one needs cost the row sweep spills), and
      // the three sums of a plain gene
      GeneSumsV<2> o2;
      lane_gene_sums<2, L, 0, STREAM>(d, c, v, a.cd, g, pre, sub, sE, sExpo, sX, stab, swin, o2);
      o2.lik = group_sum<L>(o2.lik); o2.dph = group_sum<L>(o2.dph); o2.Sr = group_sum<L>(o2.Sr);
      if (act && sub == 0) { const long G = d.G; st32(as_global(sums + 0 * G), g, o2.lik); st32(as_global(sums + 1 * G), g, o2.dph); st32(as_global(sums + 2 * G), g, o2.Sr); }
      continue;
    }
    GeneSumsV<CM> o;
    PPCX_STAMP(1);
#ifdef PPCX_TRACE
    lane_gene_sums<CM, L, GEN, STREAM>(d, c, v, a.cd, g, pre, sub, sE, sExpo, sX, stab, swin, o, (tr && tpass < kTracePasses) ? tr + tpass * kTraceStamps : nullptr);
#else
    lane_gene_sums<CM, L, GEN, STREAM>(d, c, v, a.cd, g, pre, sub, sE, sExpo, sX, stab, swin, o);
#endif
    PPCX_STAMP(2);
    // sum X_sc rho is needed of genes with slopes only (and of every gene when X[,1] != 1): a pass without such genes
    // neither reduces nor stores it (the close kernel does not use those entries of a plain gene)
    const bool with_tx = any_generic && (!d.x0_is_one || PPCX_WAVE_ANY(g < d.K));
    // every lane of the gene ends with the gene totals
    o.lik = group_sum<L>(o.lik); o.dph = group_sum<L>(o.dph); o.Sr = group_sum<L>(o.Sr);
    PPCX_STAMP(3);
    if (with_tx) {
#pragma unroll
      for (int cc = 0; cc < CM; ++cc) if (cc < d.C) o.Tx[cc] = group_sum<L>(o.Tx[cc]);
    }
    if (act && sub == 0) {
      const long G = d.G;
      st32(as_global(sums + 0 * G), g, o.lik); st32(as_global(sums + 1 * G), g, o.dph); st32(as_global(sums + 2 * G), g, o.Sr);
      if (with_tx) {
#pragma unroll
        for (int cc = 0; cc < CM; ++cc) if (cc < d.C) st32(as_global(sums + (3 + cc) * G), g, o.Tx[cc]);
      }
    }
    PPCX_STAMP(4);
#ifdef PPCX_TRACE
    ++tpass;
#endif
  }
#undef PPCX_STAMP
}

// the body of a log-likelihood workgroup: range block jb of the chain in column `col` of the launch.
// PIPE: part of a pipelined round's merged launch (ppcx_ls_kernel) -- the command in a.cmds is then the chain's command
// BEFORE the state machine that runs beside this workgroup has looked at it.
// STREAM: the per-sample constants are not staged -- the sweep reads the model's arrays in global memory (every wavefront of the
// launch walks the same few hundred KB in the same order: L1 and L2 serve them), LDS holds the two tables only
template <int CM, int GEN, bool PIPE, bool STREAM = false>
__device__ __forceinline__ void loglik_role(const LoglikArgs& a, int jb, int col, double* lds) {
  if (jb >= a.nbpc) return;
  constexpr int NS = GeneSums<CM>::N;
  const Dims& d = a.d;
  const int S = d.S, C = d.C;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  // What the workgroup stages in LDS and the wavefront's range are requested FIRST, before the chain's command is looked at
  // (three dependent scalar round trips: active list, command, its fields): the start of a launch is a chain of round trips
  // that every wavefront of the chip walks at the same time, and these need not be links of it. The first 256 (512) entries
  // travel in registers across the checks; longer per-sample arrays are completed afterwards.
  static_assert(2 * kLogTabSize == 2 * 256, "one 16-byte request per thread fills the table");
  const bool any_generic = !d.x0_is_one || (C >= 2 && d.K > 0);
  const bool evenS = (S & 1) == 0;             // then exp(exposure) is 16-byte aligned on both sides
  const int p0 = a.bounds[jb * 4 + wave], p1 = a.bounds[jb * 4 + wave + 1];
  const double2 f_tab = reinterpret_cast<const dpair_t*>(a.logtab)[tid];
  static_assert(2 * kWinTabSize == 4 * 2 * 256, "four 16-byte requests per thread fill the window table");
  double2 f_win[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) f_win[k] = reinterpret_cast<const dpair_t*>(a.wintab)[tid + 256 * k];
  double2 f_e = {0.0, 0.0};
  if (STREAM) {}
  else if (evenS) { if (tid < S / 2) f_e = reinterpret_cast<const dpair_t*>(a.sampleE)[tid]; }
  else if (tid < S) f_e.x = a.sampleE[tid];
  double f_x = 0.0;
  if (!STREAM && GEN != 2 && any_generic && tid < S) f_x = a.X[S + tid];      // the two-group path reads the group column only (C > 2: below)
  const int chain = a.active ? a.active[col] : col;
  const Cmd& c = a.cmds[chain];
  if (c.type == CMD_DONE || c.type == CMD_FLUSH) return;
  if (PIPE) {
    // evaluated and not a leaf: the gene kernel has closed it and anticipated nothing -- there is no position to evaluate
    // until the state machine has decided (a leaf that has been closed left the constants of the anticipated next leaf;
    // a command that has not been evaluated left its own)
    if (c.evaluated && c.type != CMD_LEAF) return;
  }
  double* stab = lds;                          // log table: 256 x 1/c then 256 x log c (4 KB)
  double* swin = lds + 2 * kLogTabSize;        // window table: 1024 x 1/c then 1024 x log c (16 KB)
  double* sE = swin + 2 * kWinTabSize;         // exp(exposure_s), readable kLdsPad entries past S (sweep_cells)
  // a design without the column of ones (GEN == 2) keeps the exposures and the whole of X; every other instantiation reads the
  // columns 1 .. C - 1 only: column c at sX + c S, column 0 and the exposures are not staged (the space of column 0 is sE's)
  double* sExpo = GEN == 2 ? sE + S + kLdsPad : nullptr;
  double* sX = GEN == 2 ? sExpo + S : sE + kLdsPad;      // S x C column-major, readable kLdsPad entries past its end
  const VecRef v{a.vecs + (long)chain * V_COUNT * a.Dpad, a.Dpad};
  double* sums = a.sums + (long)chain * NS * d.G;
  // the fill: every workgroup of the launch reads the same few KB at the same time, so as few requests as possible -- 16 bytes
  // per lane where the alignment allows
  reinterpret_cast<dpair_t*>(stab)[tid] = f_tab;
#pragma unroll
  for (int k = 0; k < 4; ++k) reinterpret_cast<dpair_t*>(swin)[tid + 256 * k] = f_win[k];
  if (STREAM) {}
  else if (evenS) {
    if (tid < S / 2) reinterpret_cast<dpair_t*>(sE)[tid] = f_e;
    for (int i = tid + 256; i < S / 2; i += 256) reinterpret_cast<dpair_t*>(sE)[i] = reinterpret_cast<const dpair_t*>(a.sampleE)[i];
  } else {
    if (tid < S) sE[tid] = f_e.x;
    for (int i = tid + 256; i < S; i += 256) sE[i] = a.sampleE[i];
  }
  if (!STREAM && any_generic) {
    if (GEN == 2) {
      for (int i = tid; i < S; i += 256) sExpo[i] = a.exposure[i];
      for (int i = tid; i < S * C; i += 256) sX[i] = a.X[i];
    } else {
      if (tid < S) sX[S + tid] = f_x;
      for (int i = tid + 256; i < S; i += 256) sX[S + i] = a.X[S + i];
      for (int i = 2 * S + tid; i < S * C; i += 256) sX[i] = a.X[i];      // further indicator columns (factor designs)
    }
  }
  __syncthreads();
  if (p0 >= p1) return;
  if (STREAM) { sE = const_cast<double*>(a.sampleE); sExpo = const_cast<double*>(a.exposure); sX = const_cast<double*>(a.X); }   // (read only; padded by the host)
  switch (a.lgL) {
    case 0: loglik_passes<CM, 0, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
    case 1: loglik_passes<CM, 1, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
    case 2: loglik_passes<CM, 2, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
    case 3: loglik_passes<CM, 3, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
    case 4: loglik_passes<CM, 4, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
    case 5: loglik_passes<CM, 5, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
    default: loglik_passes<CM, 6, GEN, STREAM>(a, c, v, sums, p0, p1, stab, swin, sE, sExpo, sX, lane, any_generic); break;
  }
}

template <int CM, int GEN>
__global__ __launch_bounds__(256, GEN ? PPCX_LOGLIK_OCC : PPCX_LOGLIK_OCC_FAST) void ppcx_loglik_kernel(LoglikArgs a) {
  extern __shared__ double lds[];
  // workgroups are dealt to the 8 XCDs round-robin in dispatch order: ids chain * 8 + (jb & 7) inside every run of
  // 8 range blocks x chains put the chains of one range block on ONE XCD, so its L2 fetches the rows once
  const int nch = a.nchains;
  const int lin = blockIdx.x, run = lin / (8 * nch), r = lin - run * (8 * nch);
  loglik_role<CM, GEN, false>(a, run * 8 + (r & 7), r >> 3, lds);
}

// the streamed form of the same workgroup (instantiated in ppcx_kernels_stream.hip)
template <int CM, int GEN>
__global__ __launch_bounds__(256, GEN ? PPCX_LOGLIK_OCC : PPCX_LOGLIK_OCC_FAST) void ppcx_loglik_stream_kernel(LoglikArgs a) {
  extern __shared__ double lds[];
  const int nch = a.nchains;
  const int lin = blockIdx.x, run = lin / (8 * nch), r = lin - run * (8 * nch);
  loglik_role<CM, GEN, false, true>(a, run * 8 + (r & 7), r >> 3, lds);
}

// the instantiation a model runs: CM design columns (2, 4 or 8) and which route with an exp per cell its genes can need
// (lane_gene_sums: 0 none, 1 slopes on columns of any values, 2 no column of ones)
#define PPCX_BY_CM_GEN(KERNEL, CM, GEN, EXPR)                                                                     \
  do {                                                                                                            \
    if ((CM) <= 2) { if ((GEN) == 0) { auto k_ = KERNEL<2, 0>; EXPR; } else if ((GEN) == 1) { auto k_ = KERNEL<2, 1>; EXPR; } else { auto k_ = KERNEL<2, 2>; EXPR; } } \
    else if ((CM) <= 4) { if ((GEN) == 0) { auto k_ = KERNEL<4, 0>; EXPR; } else if ((GEN) == 1) { auto k_ = KERNEL<4, 1>; EXPR; } else { auto k_ = KERNEL<4, 2>; EXPR; } } \
    else if ((CM) <= 8) { if ((GEN) == 0) { auto k_ = KERNEL<8, 0>; EXPR; } else if ((GEN) == 1) { auto k_ = KERNEL<8, 1>; EXPR; } else { auto k_ = KERNEL<8, 2>; EXPR; } } \
    else { auto k_ = KERNEL<16, 0>; EXPR; }   /* 9 .. 16 columns: indicator designs only (ppcx_model_create refuses the others) */ \
  } while (0)
// the streamed kernel of (CM, gen), for the launch helpers (ppcx_kernels.hip)
const void* loglik_stream_kernel_ptr(int CM, int gen);

}  // namespace ppcx
