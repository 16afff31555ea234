// ppcx_loo_mm.hip -- gfx950 kernels of the gene-local moment matching of PSIS-LOO cells (ppcx_fit_loo_moment_match,
// include/ppcx.h; the statistic: ppcx_loo_mm.h). The walk over the cells is ppcx_loo_dev.h's (for_gene_batches,
// cells_in_batches); the driver is ppcx_loo_mm_dev.h's loo_mm_match_cells. The argument block, the gene a workgroup reads and the
// walk's own buffers are ppcx_loo_mm_dev.h's, shared with ppcx_loo_mm_exact.hip and ppcx_loo_mm_split.hip, which run these kernels
// before their own (loo_mm_then_fit_cells); so are the stages that those kernels run too: a candidate's counted ratio sweep
// (loo_mm_count_ratios), lpd of the original draws (loo_mm_lpd) and step 4 (loo_mm_weighted_elpd).
//
//   ppcx_loo_mm_hyper_kernel  the draws' six unconstrained hyper-parameters, transposed: U[k][draw], once per call, so that a
//                             wavefront's lanes read consecutive draws of one hyper-parameter as they do of the table T.
//   ppcx_loo_mm_kernel        one workgroup of kBlockThreads per cell. ppcx_loo_kernel has run over the same cells before it
//                             and left their four fields (ppcx_fit_loo's bits, by the same kernel); a cell that is finished in
//                             step 0 copies them, writes khat_before = khat, iterations 0, scales 1, shifts 0 and leaves at
//                             once, before a ratio is formed. A cell above the threshold forms its ratios, tail and the log
//                             weight of every draw by loo_cell_ratios, loo_cell_tail and loo_cell_lw (ppcx_loo_dev.h), then
//                             Q0, and iterates: the normaliser (loo_mm_lse), per coordinate two sweeps over the draws for the
//                             four moments (t formed from the table on the fly), per candidate one sweep that forms
//                             q(t'; h) - Q0 - ll per draw (ppcx_loo_mm.h's one density under LooMmDiag) and the cell's PSIS on
//                             it. The state (A, B) and the candidate's live in LDS, written by thread 0. Every thread holds
//                             the same sums and the same k: the control flow is uniform per workgroup. Three arrays of n
//                             doubles -- a candidate's ratios, the current log weights, Q0 -- in LDS up to kPsisLdsDraws draws
//                             beside the two selection arrays (96 KB + 4 KB at 4 096 draws: one workgroup per CU; 1 000 draws
//                             take 24 KB + 2 KB), in the workgroup's slice of the bounded scratch beyond. Kept apart from
//                             ppcx_loo_mm_cov_kernel's body: as one function it was 1.6 - 2.1 % slower (profiles/README.md).
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_ap.h"

namespace ppcx {

__global__ __launch_bounds__(256) void ppcx_loo_mm_hyper_kernel(const double* draws, long n_draws, Dims d, double* U) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 6 * n_draws) return;
  const long j = t / 6; const int k = (int)(t - j * 6);
  U[(long)k * n_draws + j] = draws[j * (long)d.D + hyper_index(d, k)];
}

// AP: the cells of an ADVI fit (ppcx_loo_mm_ap.h): ppcx_loo_ap_kernel has run before it, the ratios carry a.lr, r_eff is 1
template <bool LDS, bool AP>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_kernel(LooMmArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmShared ms;
  const LooArgs& a = p.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_slice3(n));
  uint64_t* K = m.K; double* X = m.X;
  double* V = m.V;                                       // [n] the ratios (of the last candidate)
  double* W = V + n;                                     // [n] the current log weights
  double* Q0 = W + n;                                    // [n] the local density at the original draws (AP: minus a.lr)
  const LooCell c = loo_cell<false>(a);
  const int cell = c.cell, gi = c.gi, s = c.s;
  double* o = p.out + (long)cell * loo_mm_fields(C);
  const double* lo = p.loo + (long)cell * kLooFields;
  // ---- step 0: ppcx_loo_kernel's fields (AP: ppcx_loo_ap_kernel's); a finished cell leaves
  const double khat0 = lo[3];
  if (tid == 0) {
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = khat0;
    loo_mm_store_state(o, C, khat0, 0, nullptr, nullptr);
  }
  if (loo_mm_finished(c.excluded, khat0, p.k_threshold, p.max_iters)) return;
  CellRatios cr;
  if (loo_cell_ratios<false, AP>(a, c, false, V, AP ? Q0 : nullptr, sh, &cr)) return;   // (AP: ll into Q0's place until lpd is formed)
  const long N = cr.N;
  if (N == 0) return;
  double lpd, re;
  if constexpr (AP) {                                    // ppcx_loo_ap.h step 4, as ppcx_loo_ap_kernel forms it; a thread reads its own ll
    const double sl = draws_sum(n, sh.red, [&](long i) { return V[i] != -INFINITY ? exp(Q0[i] - cr.lmax) : 0.0; });
    lpd = loo_ap_lse(cr.lmax, sl) - log((double)N);
    re = 1.0;
  } else {
    lpd = loo_mm_lpd(V, n, cr, sh);
    re = a.r_eff ? a.r_eff[cell] : 1.0;
  }
  double k;
  {
    const int M = psis_tail_len(N, re);
    const LooTail lt = loo_cell_tail(V, n, N, M, K, X, a.sel_pad, sh);
    loo_cell_lw<false>(V, W, n, cr.rmax, lt, M, K, sh);
    k = lt.khat;
  }
  // ---- the gene, the state, Q0
  const LooMmGene g = loo_mm_gene(p, gi);
  if (tid < nc) { ms.A[tid] = 1.0; ms.B[tid] = 0.0; }
  __syncthreads();
  for (long i = tid; i < n; i += kBlockThreads) {
    double l;
    const double q0 = loo_mm_density(g, i, ms.A, ms.B, s, &l);
    if constexpr (AP) Q0[i] = loo_mm_ap_qa(q0, a.lr[i]);
    else Q0[i] = q0;
  }
  // ---- step 3
  int iters = 0;
  while (k > p.k_threshold && iters < p.max_iters) {
    // the normaliser of the current weights
    const double lse = loo_mm_lse(W, n, sh);
    // the moments of every coordinate, the two candidates
    bool ok2 = true;
    for (int cc = 0; cc < nc; ++cc) {
      const bool coord = loo_mm_is_coord(g, cc);           // uniform
      double A1 = ms.A[cc], B1 = ms.B[cc], A2 = A1, B2 = B1;
      if (coord) {
        double st = 0.0, swt = 0.0, swt2 = 0.0;
        for (long i = tid; i < n; i += kBlockThreads) {
          const double t = loo_mm_coord(g, cc, i, ms.A, ms.B), w = exp(W[i] - lse);
          st += t; swt += w * t; swt2 += w * (t * t);
        }
        st = block_sum(st, sh.red);
        swt = block_sum(swt, sh.red);
        swt2 = block_sum(swt2, sh.red);
        const double m = loo_mm_mean(st, n);
        double sd2 = 0.0;
        for (long i = tid; i < n; i += kBlockThreads) { const double d = loo_mm_coord(g, cc, i, ms.A, ms.B) - m; sd2 += d * d; }
        sd2 = block_sum(sd2, sh.red);
        const double v = loo_mm_var(sd2, n), vw = loo_mm_wvar(swt2, swt);
        B1 = loo_mm_shift(ms.B[cc], m, swt);
        const double sc = loo_mm_scale(vw, v);
        ok2 = ok2 && loo_mm_scale_ok(sc);
        A2 = loo_mm_scaled_A(sc, ms.A[cc]); B2 = loo_mm_scaled_B(sc, ms.B[cc], m, swt);
      }
      if (tid == 0) { ms.A1[cc] = A1; ms.B1[cc] = B1; ms.A2[cc] = A2; ms.B2[cc] = B2; }
    }
    __syncthreads();
    int kind = 0;
    for (int cand = 1; cand <= 2 && !kind; ++cand) {
      if (cand == 2 && !ok2) break;
      const double* Ac = cand == 1 ? ms.A1 : ms.A2;
      const double* Bc = cand == 1 ? ms.B1 : ms.B2;
      const CountedRatios r2 = loo_mm_count_ratios(n, V, sh, [&](long i) {
        double l;
        const double q = loo_mm_density(g, i, Ac, Bc, s, &l);
        return loo_mm_ratio(q, Q0[i], l);
      });
      const int M2 = psis_tail_len(r2.N, re);
      const LooTail lt = loo_cell_tail(V, n, r2.N, M2, K, X, a.sel_pad, sh);
      if (r2.N > 0 && lt.khat < k) {
        kind = cand; k = lt.khat;
        loo_cell_lw<false>(V, W, n, r2.rmax, lt, M2, K, sh);
        __syncthreads();
        if (tid < nc) { ms.A[tid] = Ac[tid]; ms.B[tid] = Bc[tid]; }
        __syncthreads();
      }
    }
    if (!kind) break;
    ++iters;
  }
  if (iters == 0) return;
  // ---- step 4
  const double elpd = loo_mm_weighted_elpd(W, n, sh, [&](long i) { return loo_mm_cell_ll(g, i, ms.A, ms.B, s); });
  if (tid == 0) {
    o[0] = elpd; o[1] = lpd - elpd; o[2] = -2.0 * elpd; o[3] = k;
    loo_mm_store_state(o, C, khat0, iters, ms.A, ms.B);
  }
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_kernel);

hipError_t LooMmWalk::prepare(const FitCells& fc, hipStream_t st) {
  const long n = fc.n;
  hipError_t e = U.alloc(6 * (size_t)n);
  if (e == hipSuccess) e = loo.alloc((size_t)fc.n_genes * fc.d.S * kLooFields);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ppcx_loo_mm_hyper_kernel, dim3((unsigned)((6 * n + 255) / 256)), dim3(256), 0, st, fc.draws, n, fc.d, U.p);
    e = hipGetLastError();
  }
  return e;
}
LooMmArgs LooMmWalk::args(const FitCells& fc, const LooArgs& a, const int* genes, int n_cells, double k_threshold, int max_iters,
                          double* out) {
  LooMmArgs p;
  p.l = a; p.genes = genes; p.U = U.p; p.loo = loo.p + done * kLooFields; p.K = fc.d.K; p.lambda_mu_mu = fc.d.lambda_mu_mu;
  p.k_threshold = k_threshold; p.max_iters = max_iters; p.out = out;
  p.l.out = loo.p + done * kLooFields;
  done += (size_t)n_cells;
  return p;
}
hipError_t launch_loo_mm_kernels(const LooMmArgs& q, const CellLaunch& c, hipStream_t st) {
  const hipError_t e1 = launch_loo_kernel(q.l, kLooFields, c.n_blocks, st);
  return e1 == hipSuccess ? launch_cell_kernel(pick_kernel<ppcx_loo_mm_kernel_of>(c.lds, q.l.lr != nullptr), q, c, q.l.sel_pad,
                                               loo_slice3(q.l.n), st)
                          : e1;
}

hipError_t loo_mm_fit_cells(const FitCells& fc, double k_threshold, int max_iters, double* out, size_t scratch_bytes, hipStream_t st) {
  return loo_mm_match_cells(fc, k_threshold, max_iters, loo_mm_fields(fc.d.C), out, scratch_bytes, st,
                            [&](const LooMmArgs& q, const CellLaunch& c) { return launch_loo_mm_kernels(q, c, st); });
}

}  // namespace ppcx
