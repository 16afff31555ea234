// ppcx_loo_mm_exact.hip -- gfx950 kernel of the exact leave-one-out predictive tails and interval per cell under the
// moment-matched weights (ppcx_fit_loo_predict_exact_moment_match, include/ppcx.h; the statistic: ppcx_loo_mm_exact.h). The walk
// over the cells is ppcx_loo_dev.h's (for_gene_batches, cells_in_batches); the driver at the end of this file launches, per batch
// of cells, ppcx_loo_kernel and ppcx_loo_mm_kernel as ppcx_fit_loo_moment_match does (launch_loo_mm_kernels, ppcx_loo_mm_dev.h)
// into a device record that never leaves the device, then the kernel below.
//
//   ppcx_loo_mm_exact_kernel  one workgroup of kBlockThreads per cell. It reads the cell's iterations, scale and shift from the
//                             matching's record and copies the record's tail behind its ten fields.
//                             iterations == 0: ppcx_loo_exact_kernel's own stages -- loo_cell_verdict, loo_cell_weights, (eta,
//                             ln phi) by loo_cell_eta -- so the ten fields are its bits.
//                             iterations > 0: the state (A, B) and the identity in LDS; per draw q(t; h) and Q0 by loo_mm_density
//                             in one visit (Q0 is not stored), the ratio into V; the tail and the normalised weights by
//                             loo_cell_tail and loo_cell_lw (the matching's own calls, so khat is its final khat); then
//                             (eta, ln phi) at the transformed draws, eta into the ratios' place.
//                             Both paths end in ppc_exact_sweeps over ExactBlockSums. The branch is on a value every thread of
//                             the workgroup reads from the same address: the control flow is uniform per workgroup.
//                             Three arrays of n doubles as ppcx_loo_exact_kernel -- ratio then eta, log weight then weight,
//                             ln phi -- in LDS up to kPsisLdsDraws draws beside the two selection arrays (96 KB + 4 KB at 4 096
//                             draws: one workgroup per CU; 1 000 draws take 24 KB + 2 KB), in the workgroup's slice of the
//                             bounded scratch beyond. Not timed.
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_exact.h"

namespace ppcx {

struct LooMmExactArgs {
  LooMmArgs m;                     // the matching's block: m.l the table and the cells, m.out its record [cells][loo_mm_fields(C)] (device)
  double log_tc = 0.0, p_lo = 0.025, p_hi = 0.975;
  double* out = nullptr;           // [cells][loo_mm_exact_fields(C)]
};
inline LooArgs& cell_args(LooMmExactArgs& p) { return p.m.l; }

// doubles per cell, in LDS or in the scratch: ratio / eta [n], log weight / weight [n], ln phi [n]. The matching's kernels run
// before it in slices of their own size from the same scratch, so a batch is sized by the larger of the two.
__host__ __device__ inline long loo_mm_exact_slice(long n) { return 3 * n; }

struct LooMmExactShared { double A[kMaxC + 1], B[kMaxC + 1], one[kMaxC + 1], zero[kMaxC + 1]; };

template <bool LDS>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_exact_kernel(LooMmExactArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmExactShared ms;
  const LooArgs& a = p.m.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_mm_exact_slice(n));
  double* W = m.V + n;                                   // [n] log weights, then weights (m.V: [n] the ratios)
  double* LP = W + n;                                    // [n] ln phi
  double* E = m.V;                                       // [n] eta, once the ratios are dead
  const LooCell c = loo_cell<false>(a);
  const int cell = c.cell, gi = c.gi, s = c.s, y = c.y;
  const bool excluded = c.excluded;
  double* o = p.out + (long)cell * loo_mm_exact_fields(C);
  const double* rec = p.m.out + (long)cell * loo_mm_fields(C);
  const bool matched = rec[5] > 0.0;                     // uniform: every thread reads the same word
  if (tid == 0) loo_mm_exact_store_state(o, C, rec);
  auto all_nan = [&]() { if (tid == 0) loo_exact_store_nan(o, y, excluded); };
  double khat = NAN;
  bool uniform = false, inval = false;
  if (!matched) {
    // ---- ppcx_loo_exact_kernel's stages: the ratios, the tail, the normalised weights; (eta, ln phi) of every draw
    CellRatios cr;
    const CellVerdict verdict = loo_cell_verdict<false, false>(a, c, m, nullptr, sh, &cr);
    if (verdict == CELL_NAN) { all_nan(); return; }
    uniform = verdict == CELL_UNIFORM;                   // already held out: w_i = 1, every sum over n
    if (uniform) for (long i = tid; i < n; i += kBlockThreads) W[i] = 1.0;
    else khat = loo_cell_weights<true>(a, c, m, cr, W, sh);
    __syncthreads();                                     // no thread reads a ratio any more: V becomes E
    const double* Tg = a.T + (long)gi * nc * n;
    for (long i = tid; i < n; i += kBlockThreads) {
      double sg = 0.0;
      const double eta = loo_cell_eta(a, Tg, s, i, &sg);
      const double lp = ppc_exact_lnphi(sg, p.log_tc);
      E[i] = eta; LP[i] = lp;
      inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
    }
  } else {
    // ---- the state, the ratios under it, their tail and the normalised weights; (eta, ln phi) at the transformed draws
    if (tid < nc) { ms.A[tid] = rec[kLooMmHead + tid]; ms.B[tid] = rec[kLooMmHead + nc + tid]; ms.one[tid] = 1.0; ms.zero[tid] = 0.0; }
    __syncthreads();
    const LooMmGene g = loo_mm_gene(p.m, gi);
    double cnt = 0.0, rmx = -INFINITY;
    for (long i = tid; i < n; i += kBlockThreads) {
      const double r = loo_mm_exact_ratio(g, i, ms.A, ms.B, ms.one, ms.zero, s);
      if (r != -INFINITY) { cnt += 1.0; rmx = fmax(rmx, r); }
      m.V[i] = r;
    }
    const long N = (long)block_sum(cnt, sh.red);
    rmx = block_max(rmx, sh.red);
    if (N == 0) { all_nan(); return; }
    const int M = psis_tail_len(N, a.r_eff ? a.r_eff[cell] : 1.0);
    const LooTail lt = loo_cell_tail(m.V, n, N, M, m.K, m.X, a.sel_pad, sh);
    loo_cell_lw<true>(m.V, W, n, rmx, lt, M, m.K, sh);
    khat = lt.khat;
    __syncthreads();                                     // no thread reads a ratio any more: V becomes E
    for (long i = tid; i < n; i += kBlockThreads) {
      double sg;
      const double eta = loo_mm_exact_eta(g, s, i, ms.A, ms.B, &sg);
      const double lp = ppc_exact_lnphi(sg, p.log_tc);
      E[i] = eta; LP[i] = lp;
      inval = inval || ppc_exact_invalid(eta, ppc_exact_phi(lp));
    }
  }
  if (block_any(inval)) { all_nan(); return; }
  // ---- the moments, the two tails at y, the interval (ppc_exact_sweeps); khat beside its nine fields
  const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, y, excluded, uniform ? n : 1, p.p_lo, p.p_hi, tid == 0, o);
  if (tid == 0) o[kPpcExactFields] = ok ? khat : NAN;
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_exact_kernel);

hipError_t loo_mm_exact_fit_cells(const FitCells& fc, double k_threshold, int max_iters, double tc, double p_lo, double p_hi, double* out,
                                  size_t scratch_bytes, hipStream_t st) {
  const long n = fc.n;
  const int mm_fields = loo_mm_fields(fc.d.C);
  LooMmWalk walk; DeviceBuffer<double> d_rec;            // outlive the walk, which drains the stream before it returns
  hipError_t e = walk.prepare(fc, st);
  if (e == hipSuccess) e = d_rec.alloc((size_t)fc.n_genes * fc.d.S * mm_fields);
  if (e != hipSuccess) return finish(e, st);
  const double log_tc = log(tc);
  return for_gene_batches(fc, loo_mm_exact_fields(fc.d.C), out, scratch_bytes, st,
                          [&](const LooArgs& a, const int* genes, int n_cells, DeviceBuffer<double>& scratch) {
    LooMmExactArgs p;
    const size_t done = walk.done;
    p.m = walk.args(fc, a, genes, n_cells, k_threshold, max_iters, d_rec.p + done * mm_fields);
    p.log_tc = log_tc; p.p_lo = p_lo; p.p_hi = p_hi; p.out = a.out;
    // per batch of cells: plain PSIS-LOO and the matching into the device record, then the predictive under its weights
    const long slice = loo_mm_exact_slice(n) > loo_mm_slice(n) ? loo_mm_exact_slice(n) : loo_mm_slice(n);
    return cells_in_batches(p, slice, n_cells, scratch_bytes, scratch, [&](const LooMmExactArgs& q, const CellLaunch& c) {
      const hipError_t e1 = launch_loo_mm_kernels(q.m, c, st);
      return e1 == hipSuccess ? launch_cell_kernel(pick_kernel<ppcx_loo_mm_exact_kernel_of>(c.lds), q, c, q.m.l.sel_pad, slice, st) : e1;
    });
  });
}

}  // namespace ppcx
