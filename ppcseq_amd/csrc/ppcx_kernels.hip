// ppcx_kernels.hip -- gfx950 kernels of the NB hierarchical NUTS / ADVI engine (the posterior-predictive kernels: ppcx_ppc.hip).
//
//   ppcx_loglik_kernel<CM,GEN>  streams the int32 count matrix once per gradient evaluation and reduces it to a handful
//                           of sums per gene. Replaces lp_reduce + map_rect + X*alpha of
//                           inst/stan/negBinomial_MPI.stan:58-120,:205,:226-240. CM = design columns (2, 4, 8, 16), GEN = the
//                           route with an exp per cell that is compiled in (0 none, 1 continuous covariate, 2 no column of ones).
//   ppcx_ls_kernel<CM,GEN>  the merged launch of a pipelined round: those workgroups beside the chains' state machines.
//   ppcx_gene_kernel<CM>    the other launch of a pipelined round: everything per gene (command, close, anticipated constants).
//   ppcx_disp_build_kernel  the genes' dispersion tables (ppcx_disp.h), once per model and per change of the exclusions.
//   ppcx_close_kernel<CM>   per gene: priors (.stan:219-223), gradient, second half kick of the leapfrog, NUTS tree
//                           bookkeeping of the gene's coordinates, block partial sums.
//   ppcx_step_kernel        reduction of the close kernel's block partials, hyper-parameters, NUTS / adaptation state
//                           machine (ppcx_nuts.h) and, in the same launch, the per-coordinate work of the next command.
//   ppcx_update_kernel      that per-coordinate work as a launch of its own (initialisation, ADVI).
//   ppcx_advi_kernel        the per-coordinate work of ADVI (draws, steps); ppcx_advi_elbo_kernel its ELBO.
//   ppcx_gather_kernel      column gather of the retained draws.
//
// Work decomposition of the log-likelihood kernel: a gene is owned by L lanes of one wavefront
// (L in {1,2,4,...,64}); a wavefront walks a range of the host's gene order, 64 / L genes per pass; lanes stride over the
// gene's samples four cells per trip, read the per-sample constants from LDS, and combine with an L-lane butterfly.
// Per-block partial sums of the close kernel go to a slab that the step kernel reduces in a fixed order, so results are
// bitwise reproducible for a fixed number of lanes per gene.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"
#include "ppcx_loglik.h"

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

// -----------------------------------------------------------------------------------------------------
// step kernel: one workgroup per chain.
//  phase REDUCE: fold the close kernel's slab (and the T0 slab of the previous update launch) into PT_COUNT sums in
//                a fixed order. For gene shards these per-shard sums are then added across shards (RCCL all-reduce
//                between processes, ppcx_sum_shards_kernel inside one process) before phase STEP runs.
//  phase STEP  : eight lanes of wavefront 0 run the NUTS / adaptation state machine (chain_step): lane k < 6 owns
//                hyper-parameter k, the scalar logic runs redundantly in registers, run-time-indexed arrays in LDS.
// -----------------------------------------------------------------------------------------------------
struct WaveLanes {                              // cooperating lanes 0..7 of one wavefront
  static constexpr int kPerLane = 1;
  int lane;
  __device__ __forceinline__ int k_begin() const { return lane; }
  __device__ __forceinline__ int k_end() const { return lane < 6 ? lane + 1 : lane; }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ double sum(double v) const {      // all-reduce over the 8 lanes by DPP moves (no LDS round trips)
    v += dpp_take<0xB1, 0xf>(v);               // quad_perm [1,0,3,2]: lane ^ 1
    v += dpp_take<0x4E, 0xf>(v);               // quad_perm [2,3,0,1]: lane ^ 2
    v += dpp_take<0x141, 0xf>(v);              // row_half_mirror: lane i <-> lane 7 - i, the other quad's total
    return v;
  }
  __device__ __forceinline__ double pick(const double* own, int k) const { return __shfl(own[0], k, 8); }
};

// ---- what a chain's state machine is staged with, in the step kernel and in the state-machine role of a pipelined round
struct ChainStage {                             // LDS
  double sm[3][8][32];
  double red[PT_COUNT];
  double hv[V_COUNT * 8];                      // the six hyper coordinates of every per-coordinate vector
  Cmd ex;
  ChainState st;
  Reduced rd;
};
constexpr int kStWords = (int)(sizeof(ChainState) / sizeof(int)), kCmdWords = (int)(sizeof(Cmd) / sizeof(int)), kHvDoubles = V_COUNT * 8;
static_assert(kStWords <= 4 * 256 && kCmdWords <= 256 && kHvDoubles <= 3 * 256 && PT_COUNT <= 96, "state machine staging sizes");
// the chain's state, command and hyper vectors, requested at the start and parked in registers, so that their round trip
// overlaps the reduction of the slab
struct ChainRegs { int st[4], cmd; double hv[3]; };
__device__ __forceinline__ ChainRegs chain_prefetch(const StepArgs& a, int chain, int tid) {
  ChainRegs r;
  const word_t* s2 = reinterpret_cast<const word_t*>(a.states_in + chain);
#pragma unroll
  for (int k = 0; k < 4; ++k) r.st[k] = tid + 256 * k < kStWords ? s2[tid + 256 * k] : 0;
  r.cmd = tid < kCmdWords ? reinterpret_cast<const word_t*>(a.cmds_in + chain)[tid] : 0;
  const double* hvg = a.hyper_in + (long)chain * kHvDoubles;
#pragma unroll
  for (int k = 0; k < 3; ++k) r.hv[k] = tid + 256 * k < kHvDoubles ? hvg[tid + 256 * k] : 0.0;
  return r;
}
__device__ __forceinline__ void chain_stage(const ChainRegs& r, ChainStage& s, int tid) {      // followed by a barrier
  word_t* d2 = reinterpret_cast<word_t*>(&s.st);
#pragma unroll
  for (int k = 0; k < 4; ++k) if (tid + 256 * k < kStWords) d2[tid + 256 * k] = r.st[k];
  if (tid < kCmdWords) reinterpret_cast<word_t*>(&s.ex)[tid] = r.cmd;
#pragma unroll
  for (int k = 0; k < 3; ++k) if (tid + 256 * k < kHvDoubles) s.hv[tid + 256 * k] = r.hv[k];
}
// The fold of the chain's slab into s.red, in a fixed order. One pass: thread (c, ch) sums rows ch, ch+8, ... of columns c, c+32,
// c+64, loads of several rows in flight (slab_row_groups; returns the number of sums the command produced); then, after a
// barrier, column v = sum over the eight row groups (slab_fold). All columns are loaded (stale ones included) so that these
// loads do not wait for the command that says which sums it produced; the selection happens afterwards.
// with_t0: column PT_T0 comes with the slab (the gene kernel's); otherwise it is left 0 for the T0 slab of the update launch.
__device__ __forceinline__ int slab_row_groups(const StepArgs& a, int chain, bool done, ChainStage& s, int tid) {
  const double* slab = a.partials + (long)chain * a.slab_stride * PT_COUNT;
  const int c = tid & 31, ch = tid >> 5;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const bool in2 = c + 64 < PT_COUNT;
#pragma unroll 4
  for (int b = ch; b < a.nblocks_close; b += 8) {
    const double* row = slab + (long)b * PT_COUNT;
    const double v0 = row[c], v1 = row[c + 32], v2 = in2 ? row[c + 64] : 0.0;
    s0 += v0; s1 += v1; s2 += v2;
  }
  const Cmd& exg = a.cmds_in[chain];
  const int np = (done || exg.type == CMD_DONE || exg.type == CMD_FLUSH) ? 0 : parts_used(exg);   // uniform
  s.sm[0][ch][c] = c < np ? s0 : 0.0; s.sm[1][ch][c] = c + 32 < np ? s1 : 0.0; s.sm[2][ch][c] = c + 64 < np ? s2 : 0.0;
  return np;
}
__device__ __forceinline__ void slab_fold(ChainStage& s, int np, bool with_t0, int tid) {
  if (tid < PT_COUNT) {
    double t = 0.0;
    if (tid < np && (with_t0 || tid != PT_T0)) {
#pragma unroll
      for (int k = 0; k < 8; ++k) t += s.sm[tid >> 5][k][tid & 31];
    }
    s.red[tid] = t;
  }
}
// a finished chain: its final state is carried across the double buffer
__device__ __forceinline__ void chain_carry_done(const StepArgs& a, int chain, int tid) {
  if (tid == 0) { a.states_out[chain] = a.states_in[chain]; a.cmds_out[chain] = a.cmds_in[chain]; }
  const double* hi = a.hyper_in + (long)chain * kHvDoubles;
  double* ho = a.hyper_out + (long)chain * kHvDoubles;
  for (int i = tid; i < kHvDoubles; i += 256) ho[i] = hi[i];
}
// where the chain's draws and diagnostics go (writer: the workgroup that writes what the step leaves in memory)
__device__ __forceinline__ ChainIO chain_io(const StepArgs& a, int chain, bool writer) {
  ChainIO io;
  io.draws = (writer && a.draws) ? a.draws + (long)chain * a.draws_chain_stride : nullptr;
  io.out.lp = (writer && a.out_lp) ? a.out_lp + (long)chain * a.n_keep : nullptr;
  io.out.stepsize = (writer && a.out_stepsize) ? a.out_stepsize + (long)chain * a.iter : nullptr;
  io.out.treedepth = (writer && a.out_treedepth) ? a.out_treedepth + (long)chain * a.iter : nullptr;
  io.out.n_leapfrog = (writer && a.out_n_leapfrog) ? a.out_n_leapfrog + (long)chain * a.iter : nullptr;
  io.out.divergent = (writer && a.out_divergent) ? a.out_divergent + (long)chain * a.iter : nullptr;
  io.out.accept = (writer && a.out_accept) ? a.out_accept + (long)chain * a.iter : nullptr;
  return io;
}
// after a barrier: what the step left in LDS -- hyper vectors and state -- to the other half of the double buffer (the new command
// is written from where the kernel keeps it: lane 0's registers in the step kernel, LDS in the pipelined role)
__device__ __forceinline__ void chain_write_out(const StepArgs& a, int chain, const ChainStage& s, int tid) {
  double* hvo = a.hyper_out + (long)chain * kHvDoubles;
  for (int i = tid; i < kHvDoubles; i += 256) hvo[i] = s.hv[i];
  const word_t* s2 = reinterpret_cast<const word_t*>(&s.st); word_t* d2 = reinterpret_cast<word_t*>(a.states_out + chain);
  for (int i = tid; i < kStWords; i += 256) d2[i] = s2[i];
}
// sum of v over the 256 threads of the workgroup, left in s256[0] (a binary tree over s256)
__device__ __forceinline__ void tree_sum_256(double v, double* s256, int tid) {
  s256[tid] = v;
  __syncthreads();
  for (int stp = 128; stp > 0; stp >>= 1) { if (tid < stp) s256[tid] += s256[tid + stp]; __syncthreads(); }
}

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
struct StepShared : ChainStage {
  Cmd nc;                                      // the new command: written where it is staged (step_role_pipelined)
  int x_ok[kMaxRanks]; long long x_wait;       // direct exchange: has rank k's contribution arrived; ticks waited
};
// system-scope accesses to the peer-mapped exchange buffers (uncached memory: nothing may be served from a cache line that a
// peer has rewritten since)
__device__ __forceinline__ void sys_store(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ unsigned long long sys_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// Adds the ranks' partial sums in red[0 .. PT_COUNT) (LDS), in rank order on every rank -- identical bits everywhere, so the
// replicated state machines take identical decisions. Called by all 256 threads of a chain's state-machine workgroup, red
// complete and visible. Two slots by the parity of the sequence number: a rank can be one exchange ahead of a peer (it has
// published exchange n + 1 while the peer still reads exchange n), never two, because exchange n + 2 needs the peer's n + 1.
// Returns false when a peer has aborted or does not arrive within the timeout.
__device__ __forceinline__ bool xchg_sums(const XchgArgs& x, int chain, unsigned count, StepShared& s) {
  const int tid = threadIdx.x;
  const unsigned long long seq = ((unsigned long long)x.epoch << 32) | (unsigned long long)count;
  const int slot = (int)(count & 1u);
  if (tid < PT_COUNT) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(s.red[tid]);
    for (int k = 0; k < x.nranks; ++k)
      sys_store(reinterpret_cast<unsigned long long*>(x.recv[k] + xchg_recv_index(x, slot, x.rank, chain)) + tid, bits);
  }
  __threadfence_system();                      // the sums are in the peers' memory before the sequence number is
  __syncthreads();
  if (tid < x.nranks) {
    __hip_atomic_store(x.flags[tid] + xchg_flag_index(x, slot, x.rank, chain), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long* mine = x.flags[x.rank];
    const long long t0 = (long long)wall_clock64();
    int ok = 1;
    while (__hip_atomic_load(mine + xchg_flag_index(x, slot, tid, chain), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != seq) {
      bool gone = (long long)wall_clock64() - t0 > x.timeout_ticks;
      for (int k = 0; k < x.nranks && !gone; ++k) gone = (unsigned)sys_load(mine + xchg_abort_index(x, k)) == x.epoch;
      if (gone) { ok = 0; break; }
      __builtin_amdgcn_s_sleep(4);
    }
    s.x_ok[tid] = ok;
    if (tid == 0) s.x_wait = (long long)wall_clock64() - t0;
  }
  __syncthreads();
  bool ok = true;
  for (int k = 0; k < x.nranks; ++k) ok = ok && s.x_ok[k] != 0;
  if (ok && tid < PT_COUNT) {
    double t = 0.0;
    for (int k = 0; k < x.nranks; ++k)
      t += __longlong_as_double((long long)sys_load(reinterpret_cast<const unsigned long long*>(x.recv[x.rank] + xchg_recv_index(x, slot, k, chain)) + tid));
    s.red[tid] = t;
  }
  __syncthreads();
  return ok;
}
__device__ __forceinline__ void step_role_pipelined(const StepArgs& a, int chain, StepShared& s, bool spec) {
  const int tid = threadIdx.x;
#ifdef PPCX_TESTING
  long long tr_t[7] = {0, 0, 0, 0, 0, 0, 0};
#define PPCX_SM_STAMP(k) do { tr_t[k] = (long long)wall_clock64(); } while (0)
#else
#define PPCX_SM_STAMP(k) ((void)0)
#endif
  PPCX_SM_STAMP(0);
  const bool done = a.states_in[chain].sc.phase == PH_DONE;
  const ChainRegs regs = chain_prefetch(a, chain, tid);
  // the gene kernel's slab, every column (the kinetic energy of fresh momenta arrives in column PT_T0 here); a carried
  // round reads a stale slab and ignores the sums
  const int np = slab_row_groups(a, chain, done, s, tid);
  PPCX_SM_STAMP(1);                            // the state, the command, the hyper vectors and the slab have arrived
  __syncthreads();
  slab_fold(s, np, true, tid);
  if (done) { chain_carry_done(a, chain, tid); return; }
  chain_stage(regs, s, tid);
  __syncthreads();
  PPCX_SM_STAMP(2);                            // sums folded, everything staged in LDS
  // gene shards, one per rank: the other ranks' sums. Every rank's copy of this chain reaches this point the same number of times.
  bool x_ok = true;
  const bool x_on = a.x.nranks > 1;
  if (x_on) x_ok = xchg_sums(a.x, chain, s.st.xc.count + 1u, s);
  if (tid < 8) {
    // The chain's scalars and the new command stay where they are staged, in LDS (round 5; before, lane 0's register copy was
    // written back after the step). Under the merged launch's 128-register bound that copy lived in scratch: copying it in and
    // out and reloading spilled scalars cost 3-5 of the state machine's 12-16 us per round, which bounds the launches of one and
    // two chains (profiles/r05_sm_phase_trace.txt). The eight lanes run the scalar logic redundantly on identical values, so
    // their stores to the shared copy agree -- as they always have for the tree arrays beside it. Same arithmetic: with
    // -ffp-contract=on the chains are bit for bit those of the register copy; with the default contraction the backend fuses
    // multiply-adds across statements differently when an operand passes through LDS, and a chain's rounding changes like
    // under another seed.
    ChainScalars& st = s.st.sc;
    if (x_on && tid == 0) { s.st.xc.count += 1u; s.st.xc.ticks += s.x_wait; }
    if (!x_ok) {                               // a peer has left the fit or did not arrive: this chain ends with an error
      if (tid == 0) {
        st.error = 4; st.phase = PH_DONE;
        s.nc = s.ex; s.nc.type = CMD_DONE;
        a.done[chain] = 1 + st.error;
      }
    } else {
    PPCX_SM_STAMP(3);
    (void)chain_step_pipelined(WaveLanes{tid}, a.d, st, s.st.ta, s.ex, s.red, VecRef{s.hv, 8}, chain_io(a, chain, true), s.rd, s.nc, spec);
    PPCX_SM_STAMP(4);
    if (tid == 0 && st.phase == PH_DONE) a.done[chain] = 1 + st.error;
    }
  }
#ifdef PPCX_TESTING
  if (tid == 0) {                              // phases: loads + slab, fold + staging, (exchange), state machine, and the write-out of the previous round's
    PPCX_SM_STAMP(5);
    SmTrace& tr = s.st.tr;
    tr.t[0] += tr_t[1] - tr_t[0]; tr.t[1] += tr_t[2] - tr_t[1]; tr.t[2] += tr_t[3] - tr_t[2]; tr.t[3] += tr_t[4] - tr_t[3]; tr.t[4] += tr_t[5] - tr_t[4];
    tr.n += 1;
  }
#endif
  __syncthreads();
  chain_write_out(a, chain, s, tid);
  const word_t* c2 = reinterpret_cast<const word_t*>(&s.nc); word_t* e2 = reinterpret_cast<word_t*>(a.cmds_out + chain);
  if (tid < kCmdWords) e2[tid] = c2[tid];
}

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
// The genes' dispersion tables (ppcx_disp.h), built once per model and whenever the exclusions change: one workgroup per
// gene. Phase 1: thread (panel, node) evaluates Fh and Dh at its node -- a loop over the gene's row in LDS, every thread on
// the same cell (so the y < 8 / y >= 8 branch of disp_cell is uniform). Phase 2: thread (panel, function) turns the panel's
// node values into its polynomial. 352 nodes x S cells per gene: a few milliseconds at 20 000 x 200.
// -----------------------------------------------------------------------------------------------------
constexpr int kDispThreads = 384;             // 352 nodes: one round
__global__ __launch_bounds__(kDispThreads) void ppcx_disp_build_kernel(const int* counts, int G, int S, const int* genes, int n_genes,
                                                                        DispFit fit, double* table) {
  extern __shared__ int s_row[];              // S counts, then (8-byte aligned) 2 x kDispPanels x kDispN node values
  const int gi = blockIdx.x;
  if (gi >= n_genes) return;
  const int g = genes ? genes[gi] : gi;
  const int tid = threadIdx.x;
  double* s_val = reinterpret_cast<double*>(s_row + ((S + 1) & ~1));
  for (int s = tid; s < S; s += kDispThreads) s_row[s] = counts[(long)g * S + s];
  __syncthreads();
  constexpr int NN = kDispPanels * kDispN;
  for (int t = tid; t < NN; t += kDispThreads) {
    const int p = t / kDispN, k = t - p * kDispN;
    double lo;
    const double sg = disp_node_sigma(fit, p, k, &lo);
    const DispPoint pt = disp_point(sg, lo);
    double F, D;
    disp_row(s_row, S, 0, 1, pt, &F, &D);
    s_val[(p * 2 + 0) * kDispN + k] = F; s_val[(p * 2 + 1) * kDispN + k] = D;
  }
  __syncthreads();
  for (int t = tid; t < 2 * kDispPanels; t += kDispThreads) {
    double out[kDispStride];
    disp_fit_panel(fit, s_val + t * kDispN, out);
    double* dst = table + (long)g * kDispGeneDoubles + (long)t * kDispStride;
#pragma unroll
    for (int m = 0; m < kDispStride; ++m) dst[m] = out[m];
  }
}

__global__ void ppcx_gather_kernel(const double* draws, long n_rows, int D, const int* cols, int n_cols, double* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows * n_cols) return;
  const long r = i / n_cols; const int cidx = (int)(i % n_cols);
  out[i] = draws[r * D + cols[cidx]];
}

// a rank that leaves a gene-sharded fit early (a local failure) says so to every peer: their state machines stop waiting for it
__global__ void ppcx_xchg_abort_kernel(XchgArgs x) {
  const int k = threadIdx.x;
  if (k < x.nranks) sys_store(x.flags[k] + xchg_abort_index(x, x.rank), (unsigned long long)x.epoch);
  __threadfence_system();
}

__global__ void ppcx_fill_kernel(double* p, long n, double val) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = val;
}

// -----------------------------------------------------------------------------------------------------
// launch helpers (host)
// -----------------------------------------------------------------------------------------------------
static int loglik_generic_possible(const Dims& d) { return !d.x0_is_one ? 2 : ((d.C >= 2 && d.K > 0 && !d.x1_binary) ? 1 : 0); }
// LDS of a log-likelihood workgroup: the two tables, exp(exposure_s), and the design columns its genes read -- columns 1 .. C - 1
// where X[,1] == 1 (sweep_cells: S * C doubles in all; 8 960 samples fit at C = 2), the exposures and the whole of X for a design
// without the column of ones (generic_cells: S * (2 + C))
// streamed (ppcx_model_create_ex): the tables only -- the sweep reads the per-sample constants from global memory
size_t loglik_lds_bytes(const Dims& d, bool streamed) {
  if (streamed) return sizeof(double) * (2 * kLogTabSize + 2 * kWinTabSize);
  const size_t per_sample = loglik_generic_possible(d) == 2 ? (size_t)(2 + d.C) : (size_t)(d.C < 1 ? 1 : d.C);
  return sizeof(double) * (2 * kLogTabSize + 2 * kWinTabSize + (size_t)d.S * per_sample + 2 * kLdsPad);
}
// the instantiation of a kernel that has one per number of design columns only
#define PPCX_BY_CM(KERNEL, CM) \
  ((CM) <= 2 ? (const void*)KERNEL<2> : (CM) <= 4 ? (const void*)KERNEL<4> : (CM) <= 8 ? (const void*)KERNEL<8> : (const void*)KERNEL<16>)
static const void* loglik_kernel_ptr(int CM, int gen, bool streamed) {
  if (streamed) return loglik_stream_kernel_ptr(CM, gen);
  const void* f = nullptr;
  PPCX_BY_CM_GEN(ppcx_loglik_kernel, CM, gen, f = (const void*)k_);
  return f;
}
// workgroups of 256 threads of kernel f that a CU holds with lds_bytes of dynamic LDS each (0: the query failed)
static int resident_workgroups_per_cu(const void* f, size_t lds_bytes) {
  if (lds_bytes > 64u * 1024u) {               // more than the default limit of dynamic LDS: ask for it once
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  }
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 256, lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}
int loglik_resident_workgroups_per_cu(int CM, const Dims& d, bool streamed) {
  return resident_workgroups_per_cu(loglik_kernel_ptr(CM, loglik_generic_possible(d), streamed), loglik_lds_bytes(d, streamed));
}
hipError_t launch_loglik_kernel(int CM, const LoglikArgs& a, bool streamed, hipStream_t st) {
  const size_t lds_bytes = loglik_lds_bytes(a.d, streamed);
  const dim3 grid((unsigned)((a.nbpc + 7) / 8 * 8) * (unsigned)a.nchains);
  LoglikArgs args = a;
  void* params[] = {&args};
  return hipLaunchKernel(loglik_kernel_ptr(CM, loglik_generic_possible(a.d), streamed), grid, dim3(256), params, lds_bytes, st);
}
hipError_t launch_close_kernel(int CM, const CloseArgs& a, int nblocks, int nchains, hipStream_t st) {
  CloseArgs args = a;
  void* params[] = {&args};
  return hipLaunchKernel(PPCX_BY_CM(ppcx_close_kernel, CM), dim3(nblocks, nchains), dim3(256), params, 0, st);
}
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
hipError_t launch_gene_kernel(int CM, const GeneArgs& a, int nblocks, int nchains, hipStream_t st) {
  GeneArgs args = a;
  void* params[] = {&args};
  return hipLaunchKernel(PPCX_BY_CM(ppcx_gene_kernel, CM), dim3(nblocks, nchains), dim3(256), params, 0, st);
}
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
hipError_t launch_advi_kernel(const AdviArgs& a, int nblocks, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_advi_kernel, dim3(nblocks), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_advi_elbo_kernel(const AdviElboArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_advi_elbo_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}
size_t disp_build_lds_bytes(int S) { return sizeof(int) * (size_t)((S + 1) & ~1) + sizeof(double) * 2 * kDispPanels * kDispN; }
hipError_t launch_disp_build_kernel(const int* counts, int G, int S, const int* genes, int n_genes, const DispFit& fit, double* table, hipStream_t st) {
  const size_t lds = disp_build_lds_bytes(S);
  if (lds > 64u * 1024u) {
    hipError_t e = hipFuncSetAttribute((const void*)ppcx_disp_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ppcx_disp_build_kernel, dim3((unsigned)n_genes), dim3(kDispThreads), lds, st, counts, G, S, genes, n_genes, fit, table);
  return hipGetLastError();
}
hipError_t launch_gather_kernel(const double* draws, long n_rows, int D, const int* cols, int n_cols, double* out, hipStream_t st) {
  const long n = n_rows * n_cols;
  hipLaunchKernelGGL(ppcx_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, draws, n_rows, D, cols, n_cols, out);
  return hipGetLastError();
}
hipError_t launch_xchg_abort_kernel(const XchgArgs& x, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_xchg_abort_kernel, dim3(1), dim3(64), 0, st, x);
  return hipGetLastError();
}
hipError_t launch_fill_kernel(double* p, long n, double val, hipStream_t st) {
  hipLaunchKernelGGL(ppcx_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, val);
  return hipGetLastError();
}

}  // namespace ppcx
