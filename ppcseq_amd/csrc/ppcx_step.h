// ppcx_step.h -- the chain's state machine (device), the counterpart of ppcx_loglik.h: the cooperating lanes, what a chain is staged
// with, the fold of its slab, the direct exchange of gene shards, and the state-machine role of a pipelined round -- what
// ppcx_step_kernel and ppcx_ls_kernel (both ppcx_kernels_ls.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_gene.h"
#include "ppcx_kernels.h"

namespace ppcx {

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

// ---- the state-machine role of a pipelined round (ppcx_ls_kernel)
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

}  // namespace ppcx
