// ppcx_loo_mm_cov.hip -- gfx950 kernel of gene-local moment matching with the covariance step (ppcx_fit_loo_moment_match_cov,
// include/ppcx.h; the statistic: ppcx_loo_mm_cov.h). The walk over the cells is ppcx_loo_dev.h's (for_gene_batches,
// cells_in_batches) with ppcx_loo_mm_dev.h's LooMmWalk and loo_mm_match_cells. The density is ppcx_loo_mm.h's, under the affine
// state (LooMmAffine); the normaliser, the counted ratio sweep, lpd and the weighted elpd are ppcx_loo_mm_dev.h's, shared with
// ppcx_loo_mm_kernel, whose body this one follows step for step (kept apart: ppcx_loo_mm.hip says why).
//
//   ppcx_loo_mm_cov_kernel  one workgroup of kBlockThreads per cell, after ppcx_loo_kernel over the same cells; SPLIT: the split
//                           transformation follows in the same workgroup, from the state it has just built. A cell that is
//                           finished in step 0 copies ppcx_loo_kernel's four fields, writes the identity and leaves at once.
//                           Candidate 3, reached only when 1 is refused and 2 is refused or invalid: sum w^2, then per pair
//                           (a <= b) one sweep for the two centred sums; thread
//                           0 scales them, factorises both matrices, forms L_w L^-1, L L_w^-1 and the candidate, and writes
//                           its validity to LDS; every thread reads that word behind a barrier, so the control flow is uniform
//                           per workgroup. The state (M, b), the three candidates, the accumulated inverse and the factors
//                           live in static LDS (LooMmCovShared: eight (C + 1)^2 matrices at kMaxC; 22 496 bytes with
//                           PsisShared) beside the dynamic LDS of three arrays of n doubles and the two selection arrays
//                           (96 KB + 4 KB at 4 096 draws: 124 896 of the CU's 163 840 bytes, one workgroup per CU as
//                           ppcx_loo_mm_kernel), in the workgroup's slice of the bounded scratch beyond. The inverse and logJ
//                           never leave the device. INV (ppcx_loo_mm_cov_exact.hip's driver; launched where LooMmArgs::inv
//                           is given, without SPLIT): thread 0 writes Minv, binv and logJ of a matched cell there after the
//                           loop. It is an instantiation of its own, so that the kernels of a launch without the pointer are
//                           the code they were: a run-time check of the pointer cost loo_moment_match(cov=True) 2.7 % of its time
//                           (profiles/cell_entries_ab.json, mm_cov_exact / first_version).
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_cov.h"

namespace ppcx {

// the accumulated inverse of a matched cell for the kernel that runs after this one: Minv, binv, logJ (thread 0; binv formed)
__device__ __forceinline__ void loo_mm_cov_store_inverse(double* v, int nc, const LooMmCovShared& cs) {
  for (int j = 0; j < nc * nc; ++j) v[j] = cs.Minv[j];
  for (int j = 0; j < nc; ++j) v[nc * nc + j] = cs.binv[j];
  v[nc * nc + nc] = cs.logJ;
}

template <bool LDS, bool SPLIT, bool INV = false>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_cov_kernel(LooMmArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmCovShared cs;
  const LooArgs& a = p.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem mem = cell_mem<LDS>(lds_u, a, loo_slice3(n));
  uint64_t* K = mem.K; double* X = mem.X;
  double* V = mem.V;                                     // [n] the ratios (of the last candidate; then the split's)
  double* W = V + n;                                     // [n] the current log weights (then the split's)
  double* Q0 = W + n;                                    // [n] the local density at the original draws (then the split's ll_x)
  const LooCell c = loo_cell<false>(a);
  const int cell = c.cell, gi = c.gi, s = c.s;
  double* o = p.out + (long)cell * loo_mm_cov_fields(C);
  const double* lo = p.loo + (long)cell * kLooFields;
  // ---- step 0: ppcx_loo_kernel's fields; a finished cell leaves
  const double khat0 = lo[3];
  if (tid == 0) loo_mm_cov_store(o, C, lo[0], lo[1], lo[2], khat0, khat0, 0, 0, nullptr, nullptr);
  if (loo_mm_finished(c.excluded, khat0, p.k_threshold, p.max_iters)) return;
  CellRatios cr;
  if (loo_cell_ratios<false, false>(a, c, false, V, nullptr, sh, &cr)) return;
  const long N = cr.N;
  if (N == 0) return;
  const double lpd = loo_mm_lpd(V, n, cr, sh);
  const double re = a.r_eff ? a.r_eff[cell] : 1.0;
  double k;
  {
    const int M = psis_tail_len(N, re);
    const LooTail lt = loo_cell_tail(V, n, N, M, K, X, a.sel_pad, sh);
    loo_cell_lw<false>(V, W, n, cr.rmax, lt, M, K, sh);
    k = lt.khat;
  }
  // ---- the gene, the state, Q0
  const LooMmGene g = loo_mm_gene(p, gi);
  const int d = loo_mm_cov_dim(g);
  for (int j = tid; j < nc * nc; j += kBlockThreads) { const double e = j / nc == j % nc ? 1.0 : 0.0; cs.M[j] = e; cs.Minv[j] = e; }
  if (tid < nc) cs.b[tid] = 0.0;
  if (tid == 0) cs.logJ = 0.0;
  __syncthreads();
  for (long i = tid; i < n; i += kBlockThreads) { double l; Q0[i] = loo_mm_density(g, i, LooMmAffine{cs.M, cs.b}, s, &l); }
  // ---- the loop
  int iters = 0, cov_iters = 0;
  while (k > p.k_threshold && iters < p.max_iters) {
    // the normaliser of the current weights
    const double lse = loo_mm_lse(W, n, sh);
    // the moments of every coordinate
    bool ok2 = true;
    for (int cc = 0; cc < nc; ++cc) {
      if (!loo_mm_is_coord(g, cc)) continue;               // uniform
      double st = 0.0, swt = 0.0, swt2 = 0.0;
      for (long i = tid; i < n; i += kBlockThreads) {
        const double t = loo_mm_cov_coord(g, cc, i, cs.M, cs.b), w = exp(W[i] - lse);
        st += t; swt += w * t; swt2 += w * (t * t);
      }
      st = block_sum(st, sh.red);
      swt = block_sum(swt, sh.red);
      swt2 = block_sum(swt2, sh.red);
      const double m = loo_mm_mean(st, n);
      double sd2 = 0.0;
      for (long i = tid; i < n; i += kBlockThreads) { const double dd = loo_mm_cov_coord(g, cc, i, cs.M, cs.b) - m; sd2 += dd * dd; }
      sd2 = block_sum(sd2, sh.red);
      const double sc = loo_mm_scale(loo_mm_wvar(swt2, swt), loo_mm_var(sd2, n));
      ok2 = ok2 && loo_mm_scale_ok(sc);
      if (tid == 0) { cs.m[cc] = m; cs.mw[cc] = swt; cs.sc[cc] = sc; }
    }
    // candidates 1 and 2 (thread 0 reads the moments it wrote itself)
    if (tid == 0) loo_mm_cov_cand12(g, cs.M, cs.b, cs.m, cs.mw, cs.sc, cs.b1, cs.M2, cs.b2);
    __syncthreads();
    int kind = 0;
    for (int cand = 1; cand <= 3 && !kind; ++cand) {
      if (cand == 2 && !ok2) continue;
      if (cand == 3) {
        // ---- step 5: sum w^2, the centred sums of the pairs, then thread 0
        const double sw2 = draws_sum(n, sh.red, [&](long i) { const double w = exp(W[i] - lse); return w * w; });
        for (int ia = 0; ia < d; ++ia)
          for (int ib = ia; ib < d; ++ib) {
            const int ra = loo_mm_cov_row(g, ia), rb = loo_mm_cov_row(g, ib);
            const double ma = cs.m[ra], mb2 = cs.m[rb], mwa = cs.mw[ra], mwb = cs.mw[rb];
            double sa = 0.0, sw = 0.0;
            for (long i = tid; i < n; i += kBlockThreads) {
              const double ta = loo_mm_cov_coord(g, ra, i, cs.M, cs.b), tb = loo_mm_cov_coord(g, rb, i, cs.M, cs.b);
              const double w = exp(W[i] - lse);
              sa += (ta - ma) * (tb - mb2);
              sw += w * ((ta - mwa) * (tb - mwb));
            }
            sa = block_sum(sa, sh.red);
            sw = block_sum(sw, sh.red);
            if (tid == 0) { cs.SA[ib * nc + ia] = sa; cs.SB[ib * nc + ia] = sw; }
          }
        if (tid == 0) {
          double dl = 0.0;
          cs.ok3 = loo_mm_cov_cand3(g, sw2, cs.m, cs.mw, cs.SA, cs.SB, cs.M, cs.b, cs.Tm, cs.Tinv, cs.M3, cs.b3, &dl) ? 1 : 0;
          cs.dlogJ = dl;
        }
        __syncthreads();
        if (!cs.ok3) break;                                // uniform: every thread reads the same word
      }
      const double* Mc = cand == 1 ? cs.M : cand == 2 ? cs.M2 : cs.M3;
      const double* bc = cand == 1 ? cs.b1 : cand == 2 ? cs.b2 : cs.b3;
      const CountedRatios r2 = loo_mm_count_ratios(n, V, sh, [&](long i) {
        double l;
        const double q = loo_mm_density(g, i, LooMmAffine{Mc, bc}, s, &l);
        return loo_mm_ratio(q, Q0[i], l);
      });
      const int M2 = psis_tail_len(r2.N, re);
      const LooTail lt = loo_cell_tail(V, n, r2.N, M2, K, X, a.sel_pad, sh);
      if (r2.N > 0 && lt.khat < k) {
        kind = cand; k = lt.khat;
        loo_cell_lw<false>(V, W, n, r2.rmax, lt, M2, K, sh);
        __syncthreads();                                   // no thread evaluates the density under the old state any more
        if (tid == 0) loo_mm_cov_accept_inverse(g, kind, cs.sc, cs.Tinv, cs.dlogJ, cs.Minv, &cs.logJ);
        if (cand != 1) for (int j = tid; j < nc * nc; j += kBlockThreads) cs.M[j] = Mc[j];
        if (tid < nc) cs.b[tid] = bc[tid];
        __syncthreads();
      }
    }
    if (!kind) break;
    ++iters;
    cov_iters += kind == 3 ? 1 : 0;
  }
  if (iters == 0) return;
  // ---- step 4 of ppcx_loo_mm.h
  const double elpd = loo_mm_weighted_elpd(W, n, sh, [&](long i) { return loo_mm_cell_ll(g, i, LooMmAffine{cs.M, cs.b}, s); });
  if (tid == 0) loo_mm_cov_store(o, C, elpd, lpd - elpd, -2.0 * elpd, k, khat0, iters, cov_iters, cs.M, cs.b);
  static_assert(!(INV && SPLIT), "the inverse is handed on by the non-split instantiation");
  if constexpr (INV) {
    // ---- the accumulated inverse for the kernel that runs after this one: thread 0 alone wrote Minv and logJ; binv is formed here
    if (tid == 0) {
      loo_mm_cov_binv(g, cs.Minv, cs.b, cs.binv);
      loo_mm_cov_store_inverse(p.inv + (long)cell * (nc * nc + nc + 1), nc, cs);
    }
  }
  if constexpr (SPLIT) {
    // ---- step 7: binv; candidate 2's place becomes the identity state
    __syncthreads();                                       // step 4's reads of the state and of W are over
    if (tid == 0) loo_mm_cov_binv(g, cs.Minv, cs.b, cs.binv);
    for (int j = tid; j < nc * nc; j += kBlockThreads) cs.M2[j] = j / nc == j % nc ? 1.0 : 0.0;
    if (tid < nc) cs.b2[tid] = 0.0;
    __syncthreads();
    const double logJ = cs.logJ;
    const long h = loo_mm_split_half(n);
    double* LP = Q0;                                       // [n] ll_x
    const CountedRatios sr = loo_mm_count_ratios(n, V, sh, [&](long i) {
      const bool first = i < h;
      const double* Mx = first ? cs.M : cs.M2;
      const double* bx = first ? cs.b : cs.b2;
      const double* Mi = first ? cs.M2 : cs.Minv;
      const double* bi = first ? cs.b2 : cs.binv;
      double lx;
      const double r = loo_mm_split_ratio(g, i, LooMmAffine{Mx, bx}, LooMmAffine{Mi, bi}, logJ, s, &lx);
      LP[i] = lx;
      return r;
    });
    if (sr.N == 0) { if (tid == 0) loo_mm_cov_store_split_nan(o); return; }
    const int Ms = psis_tail_len(sr.N, re);
    const LooTail lt = loo_cell_tail(V, n, sr.N, Ms, K, X, a.sel_pad, sh);
    loo_cell_lw<false>(V, W, n, sr.rmax, lt, Ms, K, sh);
    const double es = loo_mm_weighted_elpd(W, n, sh, [&](long i) { return LP[i]; });
    if (tid == 0) loo_mm_cov_store_split(o, es, lpd, lt.khat);
  }
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_cov_kernel);

// q.inv given: the non-split instantiation that leaves the accumulated inverse there (split is then not served)
hipError_t launch_loo_mm_cov_kernels(const LooMmArgs& q, const CellLaunch& c, bool split, hipStream_t st) {
  if (q.inv && split) return hipErrorInvalidValue;
  const hipError_t e1 = launch_loo_kernel(q.l, kLooFields, c.n_blocks, st);
  if (e1 != hipSuccess) return e1;
  const auto kernel = q.inv ? (c.lds ? &ppcx_loo_mm_cov_kernel<true, false, true> : &ppcx_loo_mm_cov_kernel<false, false, true>)
                            : pick_kernel<ppcx_loo_mm_cov_kernel_of>(c.lds, split);
  return launch_cell_kernel(kernel, q, c, q.l.sel_pad, loo_slice3(q.l.n), st);
}

hipError_t loo_mm_cov_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool split, double* out, size_t scratch_bytes,
                                hipStream_t st) {
  return loo_mm_match_cells(fc, k_threshold, max_iters, loo_mm_cov_fields(fc.d.C), out, scratch_bytes, st,
                            [&](const LooMmArgs& q, const CellLaunch& c) { return launch_loo_mm_cov_kernels(q, c, split, st); });
}

}  // namespace ppcx
