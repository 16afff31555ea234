// ppcx_kernels_ls.hip -- the kernels that run the chain's state machine (ppcx_step.h), in both round structures, and ADVI's:
//   ppcx_step_kernel, ppcx_update_kernel, ppcx_sum_shards_kernel, ppcx_xchg_abort_kernel   the scalar side of the three-launch round
//   ppcx_ls_kernel<CM, GEN>   the merged launch of a pipelined round: the log-likelihood workgroups (ppcx_loglik.h) beside the
//                             chains' state machines -- ten instantiations times seven lane counts, which compile beside those
//                             of ppcx_kernels.hip and ppcx_kernels_stream.hip
//   ppcx_advi_kernel, ppcx_advi_elbo_kernel
// with their launch helpers. These share one translation unit because the compiler's code for them depends on it: ppcx_step_kernel
// and ppcx_ls_kernel apart from each other, or ppcx_advi_kernel in a translation unit without them, come out with other scalar
// registers and another instruction order ("Build"; scripts/isa_kernel_diff.py shows it).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"
#include "ppcx_loglik.h"
#include "ppcx_step.h"

namespace ppcx {

// -----------------------------------------------------------------------------------------------------
// step kernel: one workgroup per chain.
//  phase REDUCE: fold the close kernel's slab (and the T0 slab of the previous update launch) into PT_COUNT sums in
//                a fixed order. For gene shards these per-shard sums are then added across shards (RCCL all-reduce
//                between processes, ppcx_sum_shards_kernel inside one process) before phase STEP runs.
//  phase STEP  : eight lanes of wavefront 0 run the NUTS / adaptation state machine (chain_step): lane k < 6 owns
//                hyper-parameter k, the scalar logic runs redundantly in registers, run-time-indexed arrays in LDS.
// -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ppcx_step_kernel(StepArgs a) {
  __shared__ ChainStage s;
  __shared__ double sT0[256];
  __shared__ Cmd s_nc;
  const int chain = blockIdx.y, tid = threadIdx.x;
  const bool lead = blockIdx.x == 0;           // with a.upd_vecs the grid has several workgroups per chain: all of them run the
                                               // step on the same inputs, the first one writes what the step leaves in memory
  const bool done = a.states_in[chain].sc.phase == PH_DONE;
  double* rg = a.red + (long)chain * PT_COUNT;
  const ChainRegs regs = chain_prefetch(a, chain, tid);
  if (a.phases & STEP_REDUCE) {
    const int np = slab_row_groups(a, chain, done, s, tid);
    __syncthreads();
    slab_fold(s, np, false, tid);
    // kinetic energy of freshly drawn momenta: only commands that drew momenta left something in the T0 slab
    const bool fresh = !done && (a.cmds_in[chain].pre_flags & (PRE_NEW_TRANSITION | PRE_EPS_TRY)) != 0;
    if (fresh) {
      const double* t0s = a.t0 + (long)chain * a.nblocks_update;
      double t = 0.0;
      for (int b = tid; b < a.nblocks_update; b += 256) t += t0s[b];
      tree_sum_256(t, sT0, tid);
      if (tid == 0) s.red[PT_T0] = sT0[0];
    }
    __syncthreads();
    if (!(a.phases & STEP_ADVANCE)) { if (lead) for (int i = tid; i < PT_COUNT; i += 256) rg[i] = s.red[i]; return; }
  } else {
    for (int i = tid; i < PT_COUNT; i += 256) s.red[i] = rg[i];     // sums completed by the shard exchange
    __syncthreads();
  }
  // ---- phase STEP
  if (done) { if (lead) chain_carry_done(a, chain, tid); return; }
  chain_stage(regs, s, tid);
  __syncthreads();
  const bool have_parts = s.st.sc.phase != PH_START;
  if (tid < 8) {
    ChainScalars st = s.st.sc;                 // scalars in registers; the run-time-indexed arrays stay in LDS
    Cmd nc;
    chain_step(WaveLanes{tid}, a.d, st, s.st.ta, s.ex, s.red, have_parts, VecRef{s.hv, 8}, chain_io(a, chain, lead), s.rd, nc);
    if (tid == 0) {
      s.st.sc = st;
      s_nc = nc;
      if (lead) {
        a.cmds_out[chain] = nc;
        if (st.phase == PH_DONE) a.done[chain] = 1 + st.error;
      }
    }
  }
  __syncthreads();
  if (lead) chain_write_out(a, chain, s, tid);
  if (!a.upd_vecs) return;
  // ---- the per-coordinate work of the command just decided
  const Dims& d = a.d;
  double T0 = 0.0;
  if (s_nc.type != CMD_DONE) {
    const VecRef v{a.upd_vecs + (long)chain * V_COUNT * a.upd_Dpad, a.upd_Dpad};
    double* draws = a.draws ? a.draws + (long)chain * a.draws_chain_stride : nullptr;
    for (int i = 3 + blockIdx.x * 256 + tid; i < d.off_tail; i += gridDim.x * 256) coord_update(d, s_nc, v, i, draws, &T0);
  }
  if ((s_nc.pre_flags & (PRE_NEW_TRANSITION | PRE_EPS_TRY)) == 0) return;
  __syncthreads();                             // sT0 was used by the reduction above
  tree_sum_256(T0, sT0, tid);
  if (tid == 0) a.upd_t0_out[(long)chain * gridDim.x + blockIdx.x] = sT0[0];
}

// in-process gene shards: every shard ends with the sum over shards (fixed order => identical bits everywhere)
__global__ void ppcx_sum_shards_kernel(ShardSumArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double s = 0.0;
  for (int k = 0; k < a.n_shards; ++k) s += a.bufs[k][i];
  for (int k = 0; k < a.n_shards; ++k) a.bufs[k][i] = s;
}

// -----------------------------------------------------------------------------------------------------
// update kernel: apply the command the step kernel just issued to every gene-owned coordinate -- proposal / sample
// copies, draw storage, Welford / metric updates, momentum refresh (Philox per coordinate), first half kick and
// drift of the next leapfrog -- and leave the kinetic energy of fresh momenta as per-workgroup partial sums.
// -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ppcx_update_kernel(UpdateArgs a) {
  __shared__ double sT0[256];
  const int chain = blockIdx.y, tid = threadIdx.x;
  const Cmd& nc = a.cmds[chain];
  const Dims& d = a.d;
  double T0 = 0.0;
  if (nc.type != CMD_DONE) {
    const VecRef v{a.vecs + (long)chain * V_COUNT * a.Dpad, a.Dpad};
    double* draws = a.draws ? a.draws + (long)chain * a.draws_chain_stride : nullptr;
    for (int i = 3 + blockIdx.x * 256 + tid; i < d.off_tail; i += gridDim.x * 256) coord_update(d, nc, v, i, draws, &T0);
  }
  // kinetic energy of freshly drawn momenta: only commands that draw momenta leave something (the step kernel's reduce
  // phase reads the slab for exactly those commands)
  if ((nc.pre_flags & (PRE_NEW_TRANSITION | PRE_EPS_TRY)) == 0) return;
  tree_sum_256(T0, sT0, tid);
  if (tid == 0) a.t0_out[(long)chain * gridDim.x + blockIdx.x] = sT0[0];
}

// a rank that leaves a gene-sharded fit early (a local failure) says so to every peer: their state machines stop waiting for it
__global__ void ppcx_xchg_abort_kernel(XchgArgs x) {
  const int k = threadIdx.x;
  if (k < x.nranks) sys_store(x.flags[k] + xchg_abort_index(x, x.rank), (unsigned long long)x.epoch);
  __threadfence_system();
}

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
hipError_t launch_step_kernel(const StepArgs& a, int nblocks, int nchains, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_step_kernel, dim3(a.upd_vecs ? nblocks : 1, nchains), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sum_shards_kernel(const ShardSumArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_sum_shards_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_update_kernel(const UpdateArgs& a, int nblocks, int nchains, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_update_kernel, dim3(nblocks, nchains), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_xchg_abort_kernel(const XchgArgs& x, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_xchg_abort_kernel, dim3(1), dim3(64), 0, st, x);
  return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------------
// Pipelined rounds: two launches per leapfrog instead of three, and the state machine off the critical path.
//   ppcx_ls_kernel   : ONE launch holds the log-likelihood workgroups of round r AND, in its first workgroups (one per
//                      chain), the state machine that digests round r - 1: it reduces the gene kernel's slab, advances
//                      the chain and writes the next command while the count matrix is being streamed. This works
//                      because the log-likelihood part reads only per-gene constants, and the gene kernel has already
//                      written those for the position the next leaf will most likely evaluate (same subtree direction,
//                      same step). When the state machine decides otherwise (a new transition, the tree turning round,
//                      the step-size search) the evaluation is void: the gene kernel then only applies the command and
//                      leaves its true constants, the next launch evaluates them, and the chain has lost one round.
//   ppcx_gene_kernel : everything that belongs to one gene, one thread per gene: the per-coordinate work of the command
//                      (what the step kernel's coordinate part does in the three-launch round), the close of the leaf,
//                      the constants of the anticipated next position.
// The three-launch round stays for gene shards (their sums cross processes between reduce and advance), ADVI,
// single evaluations and models with a per-cell linear predictor (whose cells read the positions themselves).
// -----------------------------------------------------------------------------------------------------
// Grid: runs of 8 x (chains of the launch) workgroups, as in ppcx_loglik_kernel: position r & 7 of a run is a range block,
// r >> 3 the chain's column, and the workgroups with equal r & 7 land on one XCD. In the first n_srun runs position 7 is not
// a range block but a state machine (of chain run * columns + column, if there is such a chain): state machines take the
// slot of a log-likelihood workgroup each, all on one XCD, and every workgroup of the launch is resident from its start.
template <int CM, int GEN>
__global__ __launch_bounds__(256, GEN ? PPCX_LOGLIK_OCC : PPCX_LOGLIK_OCC_FAST) void ppcx_ls_kernel(LoglikArgs a, StepArgs sa, int n_srun, int n_chains_total, int spec) {
  extern __shared__ double lds[];
  const int nch = a.nchains;
  const int lin = blockIdx.x, run = lin / (8 * nch), r = lin - run * (8 * nch);
  const int pos = r & 7, col = r >> 3;
  if (run < n_srun && pos == 7) {
    const int sc = run * nch + col;
    if (sc >= n_chains_total) return;
    __builtin_amdgcn_s_setprio(3);             // latency-bound and short: ahead of the log-likelihood wavefronts of its SIMDs
    step_role_pipelined(sa, sc, *reinterpret_cast<StepShared*>(lds), spec != 0);
    return;
  }
  const int jb = run < n_srun ? run * 7 + pos : n_srun * 7 + (run - n_srun) * 8 + pos;
  loglik_role<CM, GEN, true>(a, jb, col, lds);
}

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
static const void* ls_kernel_ptr(int CM, int gen) {
  const void* f = nullptr;
  PPCX_BY_CM_GEN(ppcx_ls_kernel, CM, gen, f = (const void*)k_);
  return f;
}
static size_t ls_lds_bytes(const Dims& d) { const size_t a = loglik_lds_bytes(d, false); return a > sizeof(StepShared) ? a : sizeof(StepShared); }
int ls_resident_workgroups_per_cu(int CM, const Dims& d) {
  return resident_workgroups_per_cu(ls_kernel_ptr(CM, loglik_generic_possible(d)), ls_lds_bytes(d));
}
hipError_t launch_ls_kernel(int CM, const LoglikArgs& a, const StepArgs& sa, int n_srun, int n_chains_total, int spec, hipStream_t st,
                            hipEvent_t ev_start, hipEvent_t ev_stop) {
  const size_t lds_bytes = ls_lds_bytes(a.d);
  // runs: the first n_srun hold 7 range blocks (and a state machine) per chain, the others 8
  int runs = n_srun;
  if (a.nbpc > 7 * n_srun) runs += (a.nbpc - 7 * n_srun + 7) / 8;
  const dim3 grid((unsigned)runs * 8u * (unsigned)a.nchains);
  LoglikArgs args = a; StepArgs sargs = sa;
  void* params[] = {&args, &sargs, &n_srun, &n_chains_total, &spec};
  if (ev_start && ev_stop)
    return hipExtLaunchKernel(ls_kernel_ptr(CM, loglik_generic_possible(a.d)), grid, dim3(256), params, lds_bytes, st, ev_start, ev_stop, 0);
  return hipLaunchKernel(ls_kernel_ptr(CM, loglik_generic_possible(a.d)), grid, dim3(256), params, lds_bytes, st);
}

// -----------------------------------------------------------------------------------------------------
// ADVI (mean-field; rstan::vb of R/utilities.R:246-278,1487-1494). The variational parameters live in spare
// vectors of slot 0: mu = V_SQ, omega = V_SG, running squared gradients = V_WM / V_WM2, initial point = V_Q0.
// One launch (a) applies the stochastic-gradient step that uses the gradient the loglik/close/reduce kernels
// just evaluated at the previous draw, and (b) writes the next Monte-Carlo draws zeta_c = mu + exp(omega) eta_c
// into the evaluation slots (V_Q1 of slot c, hyper-parameters into that slot's command).
// -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double advi_eta(uint32_t rid, uint32_t draw, uint32_t k0) {
  return coord_normal(rid, draw, 6u, 0u, k0, 0x41445649u);
}
__device__ __forceinline__ void advi_coord(const AdviArgs& a, double* mu, double* om, double* hm, double* ho,
                                            double mu0, double g, uint32_t rid) {
  if (a.op == ADVI_RESET) { *mu = mu0; *om = 0.0; *hm = 0.0; *ho = 0.0; }
  if (a.op == ADVI_STEP) {                     // Stan advi::stochastic_gradient_ascent / adapt_eta
    const double eta = advi_eta(rid, a.prev_draw, a.k0);
    const double gm = g, go = g * eta * exp(*om) + 1.0;
    if (isfinite(gm) && isfinite(go)) {        // Stan raises on a non-finite gradient; a kernel cannot: skip the draw
      *hm = a.first_iter ? gm * gm : 0.1 * gm * gm + 0.9 * *hm;
      *ho = a.first_iter ? go * go : 0.1 * go * go + 0.9 * *ho;
      *mu += a.eta_scaled * gm / (1.0 + sqrt(*hm));
      *om += a.eta_scaled * go / (1.0 + sqrt(*ho));
    }
  }
}
__global__ __launch_bounds__(256) void ppcx_advi_kernel(AdviArgs a) {
  __shared__ double s_g6[6];
  __shared__ double s_om[256];
  const Dims& d = a.d;
  const int tid = threadIdx.x;
  const VecRef v0{a.vecs, a.Dpad};
  if (a.op == ADVI_STEP && tid == 0 && blockIdx.x == 0) {   // hyper-parameter gradient of the evaluated draw
    // (only workgroup 0 owns the hyper-parameters; it rewrites cmds[] below, after the barrier)
    const Cmd& c = a.cmds[0];
    const double* r = a.red;
    double g6[6];
    (void)hyper_close(d, c.hy, c.hyp_q, r[PT_LP], r + PT_H0, g6);
    for (int k = 0; k < 6; ++k) s_g6[k] = g6[k];
  }
  __syncthreads();
  double om_sum = 0.0;
  for (int i = 3 + blockIdx.x * 256 + tid; i < d.off_tail; i += gridDim.x * 256) {
    double mu = v0.at(V_SQ, i), om = v0.at(V_SG, i), hm = v0.at(V_WM, i), ho = v0.at(V_WM2, i);
    const uint32_t rid = (uint32_t)global_flat(d, i);
    const double g = a.op == ADVI_STEP ? v0.at(V_G1, i) : 0.0;
    advi_coord(a, &mu, &om, &hm, &ho, v0.at(V_Q0, i), g, rid);
    if (a.op != ADVI_DRAW) { v0.at(V_SQ, i) = mu; v0.at(V_SG, i) = om; v0.at(V_WM, i) = hm; v0.at(V_WM2, i) = ho; }
    om_sum += om;
    const double sd = exp(om);
    for (int c = 0; c < a.n_slots; ++c) {
      const double z = mu + sd * advi_eta(rid, a.draw_base + c, a.k0);
      if (a.out_draws) a.out_draws[(long)(a.out_row0 + c) * d.D + i] = z;
      else {
        a.vecs[((long)c * V_COUNT + V_Q1) * a.Dpad + i] = z;
        coord_consts(d, VecRef{a.vecs + (long)c * V_COUNT * a.Dpad, a.Dpad}, i, z);
      }
    }
  }
  if (blockIdx.x == 0 && tid < 6) {            // the six hyper-parameters (slot 0 of the hyper vectors)
    const int k = tid, col = hyper_index(d, k);
    double* h = a.hyper;
    double mu = h[V_SQ * 8 + k], om = h[V_SG * 8 + k], hm = h[V_WM * 8 + k], ho = h[V_WM2 * 8 + k];
    const uint32_t rid = (uint32_t)global_flat(d, col);
    advi_coord(a, &mu, &om, &hm, &ho, h[V_Q0 * 8 + k], a.op == ADVI_STEP ? s_g6[k] : 0.0, rid);
    if (a.op != ADVI_DRAW) { h[V_SQ * 8 + k] = mu; h[V_SG * 8 + k] = om; h[V_WM * 8 + k] = hm; h[V_WM2 * 8 + k] = ho; }
    om_sum += om;
    const double sd = exp(om);
    for (int c = 0; c < a.n_slots; ++c) {
      const double z = mu + sd * advi_eta(rid, a.draw_base + c, a.k0);
      if (a.out_draws) a.out_draws[(long)(a.out_row0 + c) * d.D + col] = z;
      else a.cmds[c].hyp_q[k] = z;
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0 && !a.out_draws) {
    for (int c = 0; c < a.n_slots; ++c) {
      Cmd& cm = a.cmds[c];
      cm.type = CMD_EVAL; cm.dir = 1; cm.eps = 0.0; cm.pre_flags = 0; cm.n_merge = 0; cm.subtree_complete = 0; cm.leaf_n = 0;
      cm.hy = make_hyper(cm.hyp_q, d.lambda_mu_mu);
    }
  }
  s_om[tid] = om_sum;
  __syncthreads();
  for (int stp = 128; stp > 0; stp >>= 1) { if (tid < stp) s_om[tid] += s_om[tid + stp]; __syncthreads(); }
  if (tid == 0) a.omega_part[blockIdx.x] = s_om[0];
}

// ELBO accumulation: adds log p(zeta_c) of the evaluated slots (acc[0]), their count (acc[1]) and the number of
// non-finite evaluations dropped (acc[2]); acc[3] = sum of omega (entropy term) from the last advi launch.
__global__ void ppcx_advi_elbo_kernel(AdviElboArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int c = 0; c < a.n_slots; ++c) {
    const Cmd& cm = a.cmds[c];
    const double* r = a.red + (long)c * PT_COUNT;
    double g6[6];
    const double lp = hyper_close(a.d, cm.hy, cm.hyp_q, r[PT_LP], r + PT_H0, g6);
    if (isfinite(lp)) { a.acc[0] += lp; a.acc[1] += 1.0; } else a.acc[2] += 1.0;
  }
  double s = 0.0;
  for (int b = 0; b < a.n_omega_parts; ++b) s += a.omega_part[b];
  a.acc[3] = s;
}

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
hipError_t launch_advi_kernel(const AdviArgs& a, int nblocks, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_advi_kernel, dim3(nblocks), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_advi_elbo_kernel(const AdviElboArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_advi_elbo_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace ppcx
