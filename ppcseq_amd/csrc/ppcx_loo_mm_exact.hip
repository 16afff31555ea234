// ppcx_loo_mm_exact.hip -- gfx950 kernel of the exact leave-one-out predictive tails and interval per cell under the
// moment-matched weights (ppcx_fit_loo_predict_exact_moment_match, include/ppcx.h; the statistic: ppcx_loo_mm_exact.h). The walk
// over the cells is ppcx_loo_dev.h's (for_gene_batches, cells_in_batches); the driver is ppcx_loo_mm_dev.h's
// (loo_mm_then_fit_cells): per batch of cells ppcx_loo_kernel and ppcx_loo_mm_kernel as ppcx_fit_loo_moment_match launches them,
// into a device record that never leaves the device, then the kernel below.
//
//   ppcx_loo_mm_exact_kernel  one workgroup of kBlockThreads per cell. It reads the cell's iterations, scale and shift from the
//                             matching's record and copies the record's tail behind its ten fields.
//                             iterations == 0: loo_exact_cell (ppcx_loo_dev.h), the function that ppcx_loo_exact_kernel is: the
//                             ten fields are its bits by construction.
//                             iterations > 0: the state (A, B) and the identity in LDS; per draw q(t; h) and Q0 by loo_mm_density
//                             in one visit (Q0 is not stored), the ratio into V (loo_mm_count_ratios, the matching's sweep);
//                             the tail and the normalised weights by loo_cell_tail and loo_cell_lw (the matching's own calls,
//                             so khat is its final khat); then (eta, ln phi) at the transformed draws, eta into the ratios'
//                             place (loo_fill_eta_lnphi), and ppc_exact_sweeps over ExactBlockSums. The branch is on a value
//                             every thread of the workgroup reads from the same address: the control flow is uniform per
//                             workgroup.
//                             Three arrays of n doubles as ppcx_loo_exact_kernel -- ratio then eta, log weight then weight,
//                             ln phi -- in LDS up to kPsisLdsDraws draws beside the two selection arrays (96 KB + 4 KB at 4 096
//                             draws: one workgroup per CU; 1 000 draws take 24 KB + 2 KB), in the workgroup's slice of the
//                             bounded scratch beyond. Timed at the entry only (profiles/README.md, cell_entries_ab.json).
// Every reduction runs in a fixed order and a cell reads nothing of another gene: its fields are the same bits whatever else is
// requested and however the work is batched. No predictive count is drawn.
#include <hip/hip_runtime.h>
#include "ppcx_loo_mm_dev.h"
#include "ppcx_loo_mm_exact.h"
#include "ppcx_loo_mm_ap.h"

namespace ppcx {

struct LooMmExactShared { double A[kMaxC + 1], B[kMaxC + 1], one[kMaxC + 1], zero[kMaxC + 1]; };

// AP: the cells of an ADVI fit (ppcx_loo_mm_ap.h step 5): the matching's approximate-posterior instantiation has run before it,
// an unmatched cell is ppcx_loo_exact_kernel's approximate-posterior cell, a matched cell's ratios carry a.lr, r_eff is 1
template <bool LDS, bool AP>
__global__ __launch_bounds__(kBlockThreads) void ppcx_loo_mm_exact_kernel(LooMmThenArgs p) {
#pragma clang fp contract(off)
  extern __shared__ uint64_t lds_u[];
  __shared__ PsisShared sh;
  __shared__ LooMmExactShared ms;
  const LooArgs& a = p.m.l;
  const int tid = threadIdx.x;
  const long n = a.n;
  const int C = a.C, nc = C + 1;
  const CellMem m = cell_mem<LDS>(lds_u, a, loo_slice3(n));
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
  // ---- a cell that was not matched: ppcx_loo_exact_kernel's cell
  if (!matched) { loo_exact_cell<false, AP>(a, c, m, nullptr, nullptr, p.log_tc, p.p_lo, p.p_hi, o, sh); return; }
  auto all_nan = [&]() { if (tid == 0) loo_exact_store_nan(o, y, excluded); };
  // ---- the state, the ratios under it, their tail and the normalised weights; (eta, ln phi) at the transformed draws
  if (tid < nc) { ms.A[tid] = rec[kLooMmHead + tid]; ms.B[tid] = rec[kLooMmHead + nc + tid]; ms.one[tid] = 1.0; ms.zero[tid] = 0.0; }
  __syncthreads();
  const LooMmGene g = loo_mm_gene(p.m, gi);
  const CountedRatios cr = loo_mm_count_ratios(n, m.V, sh, [&](long i) {
    if constexpr (AP) return loo_mm_ap_exact_ratio(g, a.lr[i], i, ms.A, ms.B, ms.one, ms.zero, s);
    else return loo_mm_exact_ratio(g, i, ms.A, ms.B, ms.one, ms.zero, s);
  });
  if (cr.N == 0) { all_nan(); return; }
  const int M = psis_tail_len(cr.N, !AP && a.r_eff ? a.r_eff[cell] : 1.0);
  const LooTail lt = loo_cell_tail(m.V, n, cr.N, M, m.K, m.X, a.sel_pad, sh);
  loo_cell_lw<true>(m.V, W, n, cr.rmax, lt, M, m.K, sh);
  __syncthreads();                                       // no thread reads a ratio any more: V becomes E
  if (loo_fill_eta_lnphi(n, p.log_tc, E, LP, [&](long i, double* sg) { return loo_mm_exact_eta(g, s, i, ms.A, ms.B, sg); })) { all_nan(); return; }
  // ---- the moments, the two tails at y, the interval (ppc_exact_sweeps); khat beside its nine fields
  const bool ok = ppc_exact_sweeps(ExactBlockSums<true>{W, E, LP, n, sh.red}, y, excluded, 1, p.p_lo, p.p_hi, tid == 0, o);
  if (tid == 0) o[kPpcExactFields] = ok ? lt.khat : NAN;
}

// ---- launch helpers (host)
PPCX_KERNEL_OF(ppcx_loo_mm_exact_kernel);

hipError_t loo_mm_exact_fit_cells(const FitCells& fc, double k_threshold, int max_iters, double tc, double p_lo, double p_hi, double* out,
                                  size_t scratch_bytes, hipStream_t st) {
  return loo_mm_then_fit_cells(fc, LooMmDiagMatching{}, k_threshold, max_iters, tc, p_lo, p_hi, loo_mm_exact_fields(fc.d.C), out,
                               scratch_bytes, st,
                               [ap = fc.log_ratio != nullptr](bool lds) { return pick_kernel<ppcx_loo_mm_exact_kernel_of>(lds, ap); });
}

}  // namespace ppcx
