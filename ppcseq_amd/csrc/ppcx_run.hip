// ppcx_run.hip -- one run of the chains' state machines: its device scratch (Work), the launches of a round, the RCCL binding
// with the communicator and the rank guard, the pump that issues rounds until every chain is done, and the two entry points
// that are nothing but a run (ppcx_log_prob_grad; ppcx_testing_bench_kernel in the testing build).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <dlfcn.h>
#include "ppcx_host.h"

#ifdef PPCX_TRACE
static unsigned long long* g_trace_dev = nullptr;    // development builds: stamps of the log-likelihood passes (ppcx_kernels.h)
#endif
int work_alloc(Work& w, ppcx_model* m, int nchains) {
  const int D = m->d.D;
  if (!w.stream) w.stream = m->stream.s;
  w.Dpad = ((long)D + 31) / 32 * 32;
  // workgroups per chain of the step / update launches: every one of them repeats the step (reads the close kernel's
  // partial sums), so not too many, each with several coordinates per thread. The number does not depend on the chains
  // of the launch: it fixes the summation order of the kinetic energy, and a chain's results must not depend on its company.
  w.nb_update = (D + 255) / 256;
  if (w.nb_update > 80) w.nb_update = 80;
  if (w.nb_update < 1) w.nb_update = 1;
  HIPCHK(w.vecs.alloc((size_t)nchains * V_COUNT * w.Dpad));
  w.nb_close = (m->d.G + 255) / 256;
  HIPCHK(w.partials.alloc((size_t)nchains * w.nb_close * PT_COUNT));
  HIPCHK(w.sums.alloc((size_t)nchains * (3 + m->CM) * m->d.G));
  HIPCHK(hipMemsetAsync(w.sums.p, 0, sizeof(double) * (size_t)nchains * (3 + m->CM) * m->d.G, w.stream));
  HIPCHK(w.done.alloc(nchains));
  HIPCHK(w.red.alloc((size_t)nchains * PT_COUNT));
  HIPCHK(hipMemsetAsync(w.red.p, 0, sizeof(double) * (size_t)nchains * PT_COUNT, w.stream));
  HIPCHK(w.done_host.alloc(2 * nchains));     // two polls in flight (pump)
  HIPCHK(w.active_host.alloc(nchains));
  HIPCHK(w.active.alloc(nchains));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(w.hyper_vecs[i].alloc((size_t)nchains * V_COUNT * 8));
    HIPCHK(w.t0[i].alloc((size_t)nchains * w.nb_update));
    HIPCHK(w.cmds[i].alloc(nchains));
    HIPCHK(w.states[i].alloc(nchains));
    HIPCHK(hipMemsetAsync(w.hyper_vecs[i].p, 0, sizeof(double) * (size_t)nchains * V_COUNT * 8, w.stream));
    HIPCHK(hipMemsetAsync(w.t0[i].p, 0, sizeof(double) * (size_t)nchains * w.nb_update, w.stream));
    HIPCHK(hipMemsetAsync(w.cmds[i].p, 0, sizeof(Cmd) * nchains, w.stream));
    HIPCHK(hipMemsetAsync(w.states[i].p, 0, sizeof(ChainState) * nchains, w.stream));
  }
  HIPCHK(hipMemsetAsync(w.vecs.p, 0, sizeof(double) * (size_t)nchains * V_COUNT * w.Dpad, w.stream));
  HIPCHK(hipMemsetAsync(w.partials.p, 0, sizeof(double) * (size_t)nchains * w.nb_close * PT_COUNT, w.stream));
  HIPCHK(hipMemsetAsync(w.done.p, 0, sizeof(int) * nchains, w.stream));
  for (int c = 0; c < nchains; ++c) {          // inverse metric starts at identity
    HIPCHK(launch_fill_kernel(w.vecs.p + ((size_t)c * V_COUNT + V_MINV) * w.Dpad, w.Dpad, 1.0, w.stream));
    HIPCHK(launch_fill_kernel(w.hyper_vecs[0].p + ((size_t)c * V_COUNT + V_MINV) * 8, 8, 1.0, w.stream));
  }
  w.launches = 0;
  // the callers upload the initial chain states / hyper vectors next, some of them with blocking copies on the NULL
  // stream, which does not order against this non-blocking stream: the zero fills above must have landed first
  HIPCHK(hipStreamSynchronize(w.stream));
  return PPCX_OK;
}

// step kernel: reduce (+ optional) advance. After an ADVANCE launch the "current" buffers are the ones it wrote.
// The kinetic energy of freshly drawn momenta travels from the update of one round to the step of the next through the
// T0 slab, double-buffered like the states: a step launched at generation g (= w.launches) reads buffer g & 1, the
// update that belongs to the command it decides writes buffer (g + 1) & 1.
// with_update: the per-coordinate work of the new command in the same launch (ppcx_kernels_ls.hip, ppcx_step_kernel).
static void step_args(ppcx_model* m, Work& w, const RunIO& io, int phases, bool with_update, StepArgs* o) {
  const int in = (int)(w.launches & 1), out = in ^ 1;
  StepArgs& sa = *o;
  sa.d = m->d; sa.phases = phases;
  sa.states_in = w.states[in].p; sa.states_out = w.states[out].p;
  sa.cmds_in = w.cmds[in].p; sa.cmds_out = w.cmds[out].p;
  sa.hyper_in = w.hyper_vecs[in].p; sa.hyper_out = w.hyper_vecs[out].p;
  sa.partials = w.partials.p; sa.nblocks_close = w.nb_close; sa.slab_stride = w.nb_close; sa.t0 = w.t0[in].p; sa.nblocks_update = w.nb_update; sa.red = w.red.p;
  sa.draws = io.draws; sa.draws_chain_stride = io.draws_stride; sa.n_keep = io.n_keep; sa.iter = io.iter;
  sa.out_lp = io.lp; sa.out_stepsize = io.stepsize; sa.out_treedepth = io.treedepth; sa.out_n_leapfrog = io.nleap;
  sa.out_divergent = io.div; sa.out_accept = io.accept; sa.done = w.done.p;
  sa.upd_vecs = nullptr; sa.upd_Dpad = 0; sa.upd_t0_out = nullptr;
  sa.x = XchgArgs();
  if (w.xchg) {                                  // this group's chains start at xchg_chain0 of the exchange buffers
    sa.x = *w.xchg;
    sa.x.chain0 = w.xchg_chain0;
  }
  if (with_update && (phases & STEP_ADVANCE)) { sa.upd_vecs = w.vecs.p; sa.upd_Dpad = w.Dpad; sa.upd_t0_out = w.t0[out].p; }
}
int launch_step(ppcx_model* m, Work& w, int nchains, const RunIO& io, int phases, bool with_update) {
  StepArgs sa;
  step_args(m, w, io, phases, with_update, &sa);
  hipError_t e = launch_step_kernel(sa, w.nb_update, nchains, w.stream);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("step kernel: ") + hipGetErrorString(e));
  if (phases & STEP_ADVANCE) w.launches++;
  return PPCX_OK;
}
// the per-coordinate work of the current command in a launch of its own (after a step without with_update)
int launch_update(ppcx_model* m, Work& w, int nchains, const RunIO& io) {
  UpdateArgs ua;
  ua.d = m->d; ua.cmds = w.cmds[w.launches & 1].p; ua.vecs = w.vecs.p; ua.Dpad = w.Dpad;
  ua.draws = io.draws; ua.draws_chain_stride = io.draws_stride; ua.t0_out = w.t0[w.launches & 1].p;
  hipError_t e = launch_update_kernel(ua, w.nb_update, nchains, w.stream);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("update kernel: ") + hipGetErrorString(e));
  return PPCX_OK;
}
// runs of a pipelined round's merged launch whose position 7 holds state machines: one per chain of the fit, `nact`
// (chains still running = columns of the launch) per run
static int step_runs(int nchains, int nact) { return (nchains + nact - 1) / nact; }
static int loglik_args(ppcx_model* m, Work& w, int nchains, int reserve, LoglikArgs* out) {
  const int nact = w.n_active > 0 ? w.n_active : nchains;
  LoglikArgs& la = *out;
  int rc = plan_launch(m, nact, reserve, w.shared_chip, &la.nbpc, &la.bounds);
  if (rc != PPCX_OK) return rc;
  la.d = m->d; la.cd.counts = m->d_counts.p; la.cd.disp = m->d_disp.p; la.cd.gflags = m->d_gflags.p; la.cd.Sy = m->d_Sy.p; la.cd.ncell = m->d_ncell.p; la.cd.e_min = m->e_min; la.cd.e_max = m->e_max; la.sampleE = m->d_E.p; la.exposure = m->d_expo.p; la.X = m->d_X.p;
  la.vecs = w.vecs.p; la.Dpad = w.Dpad; la.cmds = w.cmds[w.launches & 1].p; la.sums = w.sums.p; la.logtab = m->d_logtab.p; la.wintab = m->d_wintab.p; la.order = m->d_order.p;
  la.lgL = 0; while ((1 << la.lgL) < m->L) ++la.lgL;
  la.nchains = nact; la.active = w.n_active > 0 ? w.active.p : nullptr;
#ifdef PPCX_TRACE
  la.trace = g_trace_dev;
#endif
  return PPCX_OK;
}
int launch_loglik(ppcx_model* m, Work& w, int nchains) {
  LoglikArgs la;
  int rc = loglik_args(m, w, nchains, 0, &la);
  if (rc != PPCX_OK) return rc;
  hipError_t e = launch_loglik_kernel(m->CM, la, m->streamed, w.stream);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("loglik kernel: ") + hipGetErrorString(e));
  return PPCX_OK;
}
static void close_args(ppcx_model* m, Work& w, CloseArgs* o) {
  CloseArgs& ca = *o;
  ca.d = m->d; ca.Sy = m->d_Sy.p; ca.SyE = m->d_SyE.p; ca.SyX = m->d_SyX.p; ca.SX = m->d_SX.p; ca.ncell = m->d_ncell.p; ca.Lg1 = m->d_Lg1.p;
  ca.sums = w.sums.p; ca.vecs = w.vecs.p; ca.Dpad = w.Dpad; ca.cmds = w.cmds[w.launches & 1].p; ca.partials = w.partials.p;
}
// pipelined round, first launch: the state machines that digest the previous gene kernel's sums beside the log-likelihood
// workgroups of this round (the command buffer the log-likelihood part reads is the one the state machines read, not
// the one they write)
static int launch_ls(ppcx_model* m, Work& w, int nchains, const RunIO& io, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
  const int nact = w.n_active > 0 ? w.n_active : nchains;
  const int n_srun = step_runs(nchains, nact);
  LoglikArgs la;
  int rc = loglik_args(m, w, nchains, n_srun * nact, &la);       // the state machines' slots are not log-likelihood workgroups
  if (rc != PPCX_OK) return rc;
  StepArgs sa;
  step_args(m, w, io, STEP_REDUCE | STEP_ADVANCE, false, &sa);
  hipError_t e = launch_ls_kernel(m->CM, la, sa, n_srun, nchains, 1, w.stream, ev_start, ev_stop);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("merged log-likelihood / step kernel: ") + hipGetErrorString(e));
  w.launches++;
  return PPCX_OK;
}
// pipelined round, second launch: the command the state machines just wrote, gene by gene
static int launch_gene_round(ppcx_model* m, Work& w, int nchains, const RunIO& io, int spec = 1) {
  GeneArgs ga;
  close_args(m, w, &ga.c);
  ga.draws = io.draws; ga.draws_chain_stride = io.draws_stride; ga.spec = spec;
  hipError_t e = launch_gene_kernel(m->CM, ga, w.nb_close, nchains, w.stream);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("gene kernel: ") + hipGetErrorString(e));
  return PPCX_OK;
}
int launch_close(ppcx_model* m, Work& w, int nchains) {
  CloseArgs ca;
  close_args(m, w, &ca);
  hipError_t e = launch_close_kernel(m->CM, ca, w.nb_close, nchains, w.stream);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("close kernel: ") + hipGetErrorString(e));
  return PPCX_OK;
}

// ---- RCCL, bound at run time (dlopen) so the library has no link-time dependency and shares the RCCL that
// the process may already have loaded (torch ships one)
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId_t;
struct RcclApi {
  void* h = nullptr;
  int (*GetUniqueId)(ncclUniqueId_t*) = nullptr;
  int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId_t, int) = nullptr;
  int (*CommDestroy)(ncclComm_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static int rccl_load() {
  if (g_rccl.h) return PPCX_OK;
#ifdef PPCX_TESTING
  // another provider of the five nccl* entry points below (tests/loopback: ranks of one host over shared memory, so that
  // the RCCL path runs with two ranks on a one-GPU box, where RCCL itself refuses two ranks on a device)
  if (!g_test.rccl_lib.empty()) {
    g_rccl.h = dlopen(g_test.rccl_lib.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!g_rccl.h) return fail(PPCX_ERR_HIP, std::string("cannot load the nccl provider ") + g_test.rccl_lib + ": " + dlerror());
  }
#endif
  if (!g_rccl.h) {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) { g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (g_rccl.h) break; }
  }
  if (!g_rccl.h) return fail(PPCX_ERR_HIP, "cannot load librccl.so");
  g_rccl.GetUniqueId = (int (*)(ncclUniqueId_t*))dlsym(g_rccl.h, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(ncclComm_t*, int, ncclUniqueId_t, int))dlsym(g_rccl.h, "ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(ncclComm_t))dlsym(g_rccl.h, "ncclCommDestroy");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t))dlsym(g_rccl.h, "ncclAllReduce");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(g_rccl.h, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce) return fail(PPCX_ERR_HIP, "librccl.so lacks the expected symbols");
  return PPCX_OK;
}
static std::string rccl_error(int e) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "error"; }
struct ppcx_comm { ncclComm_t comm = nullptr; int nranks = 1, rank = 0, device = 0; DeviceBuffer<double> d_guard; PinnedBuffer<double> h_guard; };
// What the ranks of a gene-sharded run conclude from the max-reduced guard vector [rounds, -rounds, done, -done, error]
// (a pure function: tests/test_abi.py drives it through ppcx_guard_decision without a GPU).
static int guard_decision(const double* g, int local_rc) {
  if (g[4] != 0.0) return local_rc != PPCX_OK ? local_rc : -(int)g[4];
  if (g[0] != -g[1] || g[2] != -g[3]) return PPCX_ERR_STALL;
  return PPCX_OK;
}
extern "C" int ppcx_guard_decision(const double* reduced5, int local_rc) { return reduced5 ? guard_decision(reduced5, local_rc) : PPCX_ERR_ARG; }
// Every rank of a gene-sharded run replicates the chains' state machines and must issue the same launches. At every
// poll the ranks compare (rounds issued, chains done, local error) with ONE max-reduction of [x, -x] pairs: if the
// counts differ anywhere, or any rank failed, every rank leaves the pump with the same status instead of waiting for
// a collective its peers will never issue.
static int comm_guard(ppcx_comm* c, hipStream_t st, long long pairs, int n_done, int local_rc, int* all_rc) {
  // the vector travels through pinned host memory (the device reads it in place): a failing upload cannot keep this rank
  // out of the collective its peers are about to enter
  double* v = c->h_guard.p;
  v[0] = (double)pairs; v[1] = -(double)pairs; v[2] = (double)n_done; v[3] = -(double)n_done; v[4] = local_rc != PPCX_OK ? (double)(-local_rc) : 0.0;
  const std::string local_msg = g_err;
  hipError_t he = hipMemcpyAsync(c->d_guard.p, v, sizeof(double) * 5, hipMemcpyHostToDevice, st);
  const int e = g_rccl.AllReduce(c->d_guard.p, c->d_guard.p, 5, /*ncclDouble*/ 8, /*ncclMax*/ 2, c->comm, st);
  if (e != 0) return fail(PPCX_ERR_HIP, std::string("ncclAllReduce (guard): ") + rccl_error(e));
  if (he == hipSuccess) he = hipMemcpyAsync(c->h_guard.p + 8, c->d_guard.p, sizeof(double) * 5, hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) return fail(PPCX_ERR_HIP, std::string("guard exchange: ") + hipGetErrorString(he));
  const int d = guard_decision(c->h_guard.p + 8, local_rc);
  *all_rc = d;
  if (d != PPCX_OK) {
    if (local_rc != PPCX_OK) g_err = local_msg;
    else if (d == PPCX_ERR_STALL) g_err = "the ranks of the gene-sharded run disagree on the rounds issued or the chains finished";
    else g_err = "another rank of the gene-sharded run reported an error";
  }
  return PPCX_OK;
}
// ---- one gene shard per process, sums all-reduced over RCCL -------------------------------------------
extern "C" int ppcx_comm_unique_id(char* out128) {
  if (!out128) return fail(PPCX_ERR_ARG, "NULL buffer");
  int rc = rccl_load();
  if (rc != PPCX_OK) return rc;
  ncclUniqueId_t id;
  const int e = g_rccl.GetUniqueId(&id);
  if (e != 0) return fail(PPCX_ERR_HIP, "ncclGetUniqueId failed");
  memcpy(out128, id.internal, 128);
  return PPCX_OK;
}
extern "C" int ppcx_comm_create(int device, int nranks, int rank, const char* id128, ppcx_comm** out) {
  if (!out || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(PPCX_ERR_ARG, "bad communicator arguments");
  *out = nullptr;
  int rc = rccl_load();
  if (rc != PPCX_OK) return rc;
  HIPCHK(hipSetDevice(device));
  ncclUniqueId_t id; memcpy(id.internal, id128, 128);
  ppcx_comm* c = new ppcx_comm();
  c->nranks = nranks; c->rank = rank; c->device = device;
  const int e = g_rccl.CommInitRank(&c->comm, nranks, id, rank);
  if (e != 0) { delete c; return fail(PPCX_ERR_HIP, std::string("ncclCommInitRank: ") + rccl_error(e)); }
  if (c->d_guard.alloc(8) != hipSuccess || c->h_guard.alloc(16) != hipSuccess) {
    ppcx_comm_destroy(c); return fail(PPCX_ERR_HIP, "allocating the communicator's guard buffers failed");
  }
  *out = c;
  return PPCX_OK;
}
extern "C" void ppcx_comm_destroy(ppcx_comm* c) {
  if (!c) return;
  if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
  delete c;
}

// Launch rounds until every chain reports done. A round is (loglik, close, step + update) -- three launches -- or, pipelined
// (Work::pipelined), (merged log-likelihood / step launch, gene kernel) -- two. With several shards in one process they share
// shard 0's stream and their partial sums are added by ppcx_sum_shards_kernel; with a communicator the sums are all-reduced
// over the ranks (RCCL, xGMI) between reduce and advance.
int pump(std::vector<Shard>& sh, int nchains, ppcx_comm* comm, long long max_pairs, bool time_kernels, PumpStats* stats) {
  const int ns = (int)sh.size();
  hipStream_t st = sh[0].w->stream;
  int rc = PPCX_OK;
  // Several ranks (one gene shard per process): a rank that fails must not leave its peers waiting in a collective. It
  // stops launching kernels but keeps issuing the per-round all-reduces until the next poll, where comm_guard lets every
  // rank see the failure (or a disagreement on the rounds issued) and leave together. Every local failure inside the
  // loop -- a launch, an event, a copy -- becomes local_rc; only a failing collective returns at once (its peers are
  // then in an undefined state anyway).
  const bool guarded = comm && comm->comm && comm->nranks > 1;
  const bool piped = ns == 1 && !(comm && comm->comm) && sh[0].w->pipelined;
  int local_rc = PPCX_OK;
#define PUMP_TRY(expr) do { if (local_rc == PPCX_OK) { const int r_ = (expr); if (r_ != PPCX_OK) { if (!guarded) return r_; local_rc = r_; } } } while (0)
#define PUMP_HIP(expr) do { if (local_rc == PPCX_OK) { const hipError_t e_ = (expr); if (e_ != hipSuccess) { const int r_ = fail(PPCX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); if (!guarded) return r_; local_rc = r_; } } } while (0)
  if (!piped) for (int k = 0; k < ns; ++k) {                      // PH_START: first command, then its coordinate work
    PUMP_TRY(launch_step(sh[k].m, *sh[k].w, nchains, sh[k].io, STEP_REDUCE | STEP_ADVANCE));
    PUMP_TRY(launch_update(sh[k].m, *sh[k].w, nchains, sh[k].io));
  }
  const int batch = 32, sample_every = 16;
  struct Events {                // destroyed on every exit path
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } evs;
  if (time_kernels) for (int i = 0; i < 4; ++i) if (hipEventCreate(&evs.e[i]) != hipSuccess) { evs.e[i] = nullptr; time_kernels = false; }
  hipEvent_t &ev0 = evs.e[0], &ev1 = evs.e[1], &ev2 = evs.e[2], &ev3 = evs.e[3];
  // The poll. Plain: after every batch of rounds the done flags are copied back and the stream is waited for -- the GPU then
  // idles until the host has woken up and launched again. A pipelined single-process fit polls ONE BATCH BEHIND instead: the
  // flags of batch b are looked at while batch b + 1 is already queued, so the queue never runs dry (single stream: 2 % of a
  // fit were such bubbles). The chains notice one batch later that they are all done (32 rounds of kernels that return at
  // once), and the list of active chains is still rewritten on an idle stream, a few times per fit.
  bool lookahead = piped && !guarded;
  if (lookahead) for (int i = 4; i < 6; ++i) if (hipEventCreateWithFlags(&evs.e[i], hipEventDisableTiming) != hipSuccess) { evs.e[i] = nullptr; lookahead = false; }
  long long pairs = 0; int n_done = 0, n_done_applied = 0;
  const auto t_start = std::chrono::steady_clock::now(); auto t_report = t_start;
  Work& w0 = *sh[0].w;
  int cur = 0; bool have_prev = false, sampled_prev = false;
  while (true) {
    bool sampled = false;
    for (int i = 0; i < batch; ++i, ++pairs) {
      const bool smp = time_kernels && !sampled && (pairs / batch) % sample_every == 0 && i == batch / 2 && local_rc == PPCX_OK;
      if (smp && !piped) PUMP_HIP(hipEventRecord(ev0, st));
      if (piped) {
        // a sampled merged launch carries its own start / stop events (hipExtLaunchKernel): the kernel's duration as the
        // profiler's kernel trace sees it; a hipEventRecord on either side adds its marker packets (3-4 us on a 38 us launch)
        PUMP_TRY(launch_ls(sh[0].m, w0, nchains, sh[0].io, smp ? ev0 : nullptr, smp ? ev1 : nullptr));
        if (smp) sampled = true;
        PUMP_TRY(launch_gene_round(sh[0].m, w0, nchains, sh[0].io));
        if (smp) { PUMP_HIP(hipEventRecord(ev2, st)); PUMP_HIP(hipEventRecord(ev3, st)); }
        continue;
      }
      for (int k = 0; k < ns; ++k) PUMP_TRY(launch_loglik(sh[k].m, *sh[k].w, nchains));
      if (smp) { PUMP_HIP(hipEventRecord(ev1, st)); sampled = true; }
      const bool exchange = ns > 1 || (comm && comm->comm);
      for (int k = 0; k < ns; ++k) {
        PUMP_TRY(launch_close(sh[k].m, *sh[k].w, nchains));
        if (smp && k == ns - 1) PUMP_HIP(hipEventRecord(ev2, st));
        PUMP_TRY(launch_step(sh[k].m, *sh[k].w, nchains, sh[k].io, exchange ? STEP_REDUCE : (STEP_REDUCE | STEP_ADVANCE), !exchange));
      }
      if (ns > 1) {
        ShardSumArgs sa; sa.n_shards = ns; sa.n = nchains * PT_COUNT;
        for (int k = 0; k < ns; ++k) sa.bufs[k] = sh[k].w->red.p;
        PUMP_HIP(launch_sum_shards_kernel(sa, st));
      }
      if (comm && comm->nranks >= 1 && comm->comm) {                 // issued by every rank every round, failed or not
        const int e = g_rccl.AllReduce(w0.red.p, w0.red.p, (size_t)nchains * PT_COUNT, /*ncclDouble*/ 8, /*ncclSum*/ 0, comm->comm, st);
        if (e != 0) return fail(PPCX_ERR_HIP, std::string("ncclAllReduce: ") + rccl_error(e));
      }
      for (int k = 0; k < ns; ++k) {
        if (exchange) PUMP_TRY(launch_step(sh[k].m, *sh[k].w, nchains, sh[k].io, STEP_ADVANCE, true));   // step + coordinate update in one launch
      }
      if (smp) PUMP_HIP(hipEventRecord(ev3, st));
    }
#ifdef PPCX_TESTING
    if (g_test.fail_at_round > 0 && pairs >= g_test.fail_at_round && local_rc == PPCX_OK &&
        (g_test.fail_rank < 0 || (!comm && !w0.xchg) || g_test.fail_rank == (comm ? comm->rank : w0.xchg->rank)))   // fault injection
      local_rc = fail(PPCX_ERR_HIP, "injected failure (ppcx_testing_set fail_at_round)");
#endif
    int* flags = w0.done_host.p + (lookahead ? cur * nchains : 0);
    PUMP_HIP(hipMemcpyAsync(flags, w0.done.p, sizeof(int) * nchains, hipMemcpyDeviceToHost, st));
    bool sampled_chk = sampled;
    if (lookahead) {
      PUMP_HIP(hipEventRecord(evs.e[4 + cur], st));
      if (!have_prev) { have_prev = true; sampled_prev = sampled; cur ^= 1; continue; }   // the first batch is looked at after the second is queued
      flags = w0.done_host.p + (cur ^ 1) * nchains;
      PUMP_HIP(hipEventSynchronize(evs.e[4 + (cur ^ 1)]));
      sampled_chk = sampled_prev; sampled_prev = sampled;
    } else {
      PUMP_HIP(hipStreamSynchronize(st));
    }
    if (sampled_chk && n_done == 0 && local_rc == PPCX_OK) {   // only launches in which every chain was still active
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) {
        stats->kA_ms_sum += ms; stats->kA_samples++; stats->chain_launches += nchains;
        if (hipEventElapsedTime(&ms, ev1, ev2) == hipSuccess) stats->kC_ms_sum += ms;
        if (hipEventElapsedTime(&ms, ev2, ev3) == hipSuccess) stats->kU_ms_sum += ms;
      }
    }
    n_done = 0;
    rc = local_rc;
    if (local_rc == PPCX_OK) for (int c = 0; c < nchains; ++c) {
      if (flags[c]) ++n_done;
      if (flags[c] == 2) rc = fail(PPCX_ERR_INIT, "no finite initial point after 100 attempts");
      if (flags[c] == 3) rc = fail(PPCX_ERR_STEPSIZE, "step-size heuristic diverged");
      if (flags[c] == 5) rc = fail(PPCX_ERR_STALL, "gene-shard exchange: a peer rank left the fit or did not arrive within the timeout");
    }
    if (pairs > max_pairs && n_done < nchains && rc == PPCX_OK) rc = fail(PPCX_ERR_STALL, "launch budget exhausted before the chains finished");
    if (guarded) {
      int all_rc = PPCX_OK;
      const int grc = comm_guard(comm, st, pairs, n_done, rc, &all_rc);
      if (grc != PPCX_OK) return grc;
      if (all_rc != PPCX_OK) { rc = all_rc; break; }
    } else if (rc != PPCX_OK) break;
    if (sh[0].m->progress && local_rc == PPCX_OK) {   // a blocking call of minutes need not be silent: rounds issued, chains done
      const auto now = std::chrono::steady_clock::now();
      if (std::chrono::duration<double>(now - t_report).count() >= sh[0].m->progress_every || n_done == nchains) {
        t_report = now;
        const int stop = sh[0].m->progress(sh[0].m->progress_user, sh[0].w->xchg_chain0, nchains, n_done, pairs, std::chrono::duration<double>(now - t_start).count());
        if (stop != 0 && n_done < nchains) {     // the caller's budget is spent: a local failure like any other
          local_rc = fail(PPCX_ERR_CANCELLED, "the progress callback ended the fit");
          if (w0.stop) w0.stop->store(1);
          if (!guarded) { rc = local_rc; break; }
        }
      }
    }
    if (w0.stop && w0.stop->load() && local_rc == PPCX_OK && n_done < nchains) {   // another chain group of this fit was ended
      local_rc = fail(PPCX_ERR_CANCELLED, "the progress callback ended the fit");
      if (!guarded) { rc = local_rc; break; }
    }
    if (n_done == nchains) break;
    // fewer chains in the launch: the others get their wavefronts (the list is rewritten on an idle stream: with the poll one
    // batch behind the queued batch is waited for first, and its newer flags are the ones applied)
    if (n_done > n_done_applied) {
      if (lookahead) {
        PUMP_HIP(hipStreamSynchronize(st));
        flags = w0.done_host.p + cur * nchains;
        have_prev = false;                       // both batches are finished and looked at: start over
      }
      int na = 0;
      for (int c = 0; c < nchains; ++c) if (!flags[c]) w0.active_host.p[na++] = c;
      n_done_applied = nchains - na;
      if (na == 0) { n_done = nchains; break; }
      for (int k = 0; k < ns; ++k) {
        Work& wk = *sh[k].w;
        PUMP_HIP(hipMemcpyAsync(wk.active.p, w0.active_host.p, sizeof(int) * na, hipMemcpyHostToDevice, st));
        wk.n_active = na;
      }
      PUMP_HIP(hipStreamSynchronize(st));
    }
    if (lookahead) cur ^= 1;
  }
  if (lookahead) (void)hipStreamSynchronize(st);   // a queued batch may still be running: nothing is freed under it
#undef PUMP_TRY
#undef PUMP_HIP
  stats->pairs = pairs;
  return rc;
}
int pump(ppcx_model* m, Work& w, int nchains, const RunIO& io, long long max_pairs, bool time_kernels, PumpStats* stats,
         ppcx_comm* comm) {
  std::vector<Shard> sh(1);
  sh[0].m = m; sh[0].w = &w; sh[0].io = io;
  return pump(sh, nchains, comm, max_pairs, time_kernels, stats);
}

extern "C" int ppcx_log_prob_grad(ppcx_model* m, int n_points, const double* u, double* lp, double* grad) {
  if (!m || n_points < 1 || !u || !lp) return fail(PPCX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(m->device));
  const int D = m->d.D;
  const int maxb = 256;                         // points per batch (grid.y)
  for (int p0 = 0; p0 < n_points; p0 += maxb) {
    const int nb = n_points - p0 < maxb ? n_points - p0 : maxb;
    choose_launch(m, nb);
    Work w;
    int rc = work_alloc(w, m, nb);
    if (rc != PPCX_OK) return rc;
    std::vector<ChainState> states(nb);
    NutsConfig cfg; memset(&cfg, 0, sizeof cfg);
    cfg.chains = nb; cfg.iter = 0; cfg.warmup = 0; cfg.seed = 0; cfg.adapt_delta = 0.8; cfg.max_treedepth = 10;
    cfg.init_radius = 2; cfg.stepsize0 = 1; cfg.init_buffer = 75; cfg.term_buffer = 50; cfg.window = 25; cfg.chain_id_offset = 0;
    for (int c = 0; c < nb; ++c) state_init(states[c], cfg, c, 1);
    HIPCHK(hipMemcpyAsync(w.states[0].p, states.data(), sizeof(ChainState) * nb, hipMemcpyHostToDevice, m->stream.s));
    std::vector<double> hq((size_t)nb * V_COUNT * 8, 0.0);
    for (int c = 0; c < nb; ++c) {
      const double* uc = u + (size_t)(p0 + c) * D;
      HIPCHK(hipMemcpyAsync(w.vecs.p + ((size_t)c * V_COUNT + V_Q1) * w.Dpad, uc, sizeof(double) * D, hipMemcpyHostToDevice, m->stream.s));
      for (int k = 0; k < 6; ++k) hq[((size_t)c * V_COUNT + V_Q1) * 8 + k] = uc[hyper_index(m->d, k)];
      for (int k = 0; k < 8; ++k) hq[((size_t)c * V_COUNT + V_MINV) * 8 + k] = 1.0;
    }
    HIPCHK(hipMemcpyAsync(w.hyper_vecs[0].p, hq.data(), sizeof(double) * hq.size(), hipMemcpyHostToDevice, m->stream.s));
    RunIO io;
    PumpStats ps;
    rc = pump(m, w, nb, io, 64, false, &ps);
    if (rc != PPCX_OK) return rc;
    HIPCHK(hipMemcpy(states.data(), current_states(w), sizeof(ChainState) * nb, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hq.data(), current_hyper(w), sizeof(double) * hq.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < nb; ++c) {
      lp[p0 + c] = states[c].sc.lp_eval;
      if (grad) {
        double* gc = grad + (size_t)(p0 + c) * D;
        HIPCHK(hipMemcpy(gc, w.vecs.p + ((size_t)c * V_COUNT + V_G1) * w.Dpad, sizeof(double) * D, hipMemcpyDeviceToHost));
        for (int k = 0; k < 6; ++k) gc[hyper_index(m->d, k)] = hq[((size_t)c * V_COUNT + V_G1) * 8 + k];
      }
    }
  }
  return PPCX_OK;
}

#ifdef PPCX_TESTING
// ---- testing build only (ppcx_testing.h) ---------------------------------------------------------------------------
extern "C" int ppcx_testing_set_nccl_provider(const char* path) {
  if (g_rccl.h) return fail(PPCX_ERR_ARG, "the nccl entry points are bound already");
  g_test.rccl_lib = path ? path : "";
  return PPCX_OK;
}
static int launch_gene(ppcx_model* m, Work& w, int nchains) {   // one gradient evaluation = loglik + close
  int rc = launch_loglik(m, w, nchains);
  return rc != PPCX_OK ? rc : launch_close(m, w, nchains);
}
// Kernel-level timing: mean duration (ms) of `reps` back-to-back launches of one kernel (`which`, ppcx_testing.h) of the
// three-launch round on the command the chains hold after `warm_rounds` rounds of a real run. n_merge >= 0 overrides the
// tree position of that command (number of subtree merges the leaf closes), so every variant is timed on the same work.
extern "C" int ppcx_testing_bench_kernel(ppcx_model* m, int which, int nchains, int warm_rounds, int reps, int n_merge,
                                         double* ms_per_launch, int* cmd_type) {
  if (!m || nchains < 1 || reps < 1 || !ms_per_launch || which < 0 || which > PPCX_BENCH_GENE_NEW_TRANSITION) return fail(PPCX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(m->device));
  choose_launch(m, nchains);
  Work w;
  int rc = work_alloc(w, m, nchains);
  if (rc != PPCX_OK) return rc;
  NutsConfig nc; memset(&nc, 0, sizeof nc);
  nc.chains = nchains; nc.iter = 1000000; nc.warmup = 1000000; nc.seed = 1; nc.adapt_delta = 0.8; nc.max_treedepth = 10;
  nc.init_radius = 2; nc.stepsize0 = 1; nc.init_buffer = 75; nc.term_buffer = 50; nc.window = 25;
  std::vector<ChainState> states(nchains);
  for (int c = 0; c < nchains; ++c) state_init(states[c], nc, c, 0);
  HIPCHK(hipMemcpyAsync(w.states[0].p, states.data(), sizeof(ChainState) * nchains, hipMemcpyHostToDevice, m->stream.s));
  RunIO io; io.iter = nc.iter;
  hipStream_t st = m->stream.s;
  if ((rc = launch_step(m, w, nchains, io, STEP_REDUCE | STEP_ADVANCE)) != PPCX_OK) return rc;
  if ((rc = launch_update(m, w, nchains, io)) != PPCX_OK) return rc;
  for (int i = 0; i < warm_rounds; ++i) {
    if ((rc = launch_gene(m, w, nchains)) != PPCX_OK) return rc;
    if ((rc = launch_step(m, w, nchains, io, STEP_REDUCE | STEP_ADVANCE)) != PPCX_OK) return rc;
    if ((rc = launch_update(m, w, nchains, io)) != PPCX_OK) return rc;
  }
  HIPCHK(hipStreamSynchronize(st));
  Cmd* dcmds = w.cmds[w.launches & 1].p;
  std::vector<Cmd> cmds(nchains);
  HIPCHK(hipMemcpy(cmds.data(), dcmds, sizeof(Cmd) * nchains, hipMemcpyDeviceToHost));
  if (cmd_type) *cmd_type = cmds[0].type;
  if (n_merge >= 0) for (int c = 0; c < nchains; ++c) {
    // a chain still searching its step size after the warm rounds is timed on a leaf as well (the gene kernel's variants:
    // with step-size trials among the chains the launch takes as long as their fresh momenta, whatever the others do)
    if (which >= PPCX_BENCH_GENE && cmds[c].type == CMD_EPS_TRY) { cmds[c].type = CMD_LEAF; cmds[c].pre_dir = cmds[c].dir; cmds[c].next_dir = cmds[c].dir; cmds[c].leaf_n = 1; }
    if (cmds[c].type != CMD_LEAF) continue;
    cmds[c].n_merge = n_merge; cmds[c].subtree_complete = 0;
    cmds[c].eps *= 1e-3;                         // keep the repeated second half kicks on a bounded trajectory
  }
  if (which >= PPCX_BENCH_GENE) for (int c = 0; c < nchains; ++c) {   // the gene kernel of a pipelined round: apply + close + anticipate
    cmds[c].evaluated = 1; cmds[c].updated = 0;
    // a plain leaf inside a subtree: the proposal copy is its only pre-operation (the command left by the warm rounds may be a
    // transition's first leaf, whose fresh momenta -- Philox, Box-Muller -- are a thirtieth of a fit's rounds, not the typical one)
    if (cmds[c].type == CMD_LEAF) { cmds[c].pre_flags = PRE_PROP; cmds[c].prop_slot = n_merge >= 0 ? n_merge : 0; cmds[c].prop_src = -1; }
    if (which == PPCX_BENCH_GENE_NEW_TRANSITION && cmds[c].type == CMD_LEAF) { cmds[c].pre_flags = PRE_NEW_TRANSITION | PRE_SAVE_NEAR; cmds[c].rng_c1 = 7; }
    if (which == PPCX_BENCH_GENE_NO_PROP) cmds[c].pre_flags &= ~PRE_PROP;   // what the kernel would cost without the proposal copies
    if (which == PPCX_BENCH_GENE_UPDATE_ONLY) cmds[c].evaluated = 0;        // apply the command only (no close, its own constants)
  }
  HIPCHK(hipMemcpy(dcmds, cmds.data(), sizeof(Cmd) * nchains, hipMemcpyHostToDevice));
  auto one = [&]() -> int {
    switch (which) {
      case PPCX_BENCH_CLOSE: return launch_close(m, w, nchains);
      case PPCX_BENCH_LOGLIK_CLOSE: return launch_gene(m, w, nchains);
      case PPCX_BENCH_STEP: return launch_step(m, w, nchains, io, STEP_REDUCE | STEP_ADVANCE);
      case PPCX_BENCH_UPDATE: return launch_update(m, w, nchains, io);
      case PPCX_BENCH_STEP_REDUCE: return launch_step(m, w, nchains, io, STEP_REDUCE);
      case PPCX_BENCH_STEP_ADVANCE: return launch_step(m, w, nchains, io, STEP_ADVANCE);
      case PPCX_BENCH_STEP_UPDATE: return launch_step(m, w, nchains, io, STEP_REDUCE | STEP_ADVANCE, true);
      case PPCX_BENCH_GENE: case PPCX_BENCH_GENE_NO_PROP: case PPCX_BENCH_GENE_UPDATE_ONLY: case PPCX_BENCH_GENE_NEW_TRANSITION:
        return launch_gene_round(m, w, nchains, io);
      case PPCX_BENCH_GENE_NO_SPEC: return launch_gene_round(m, w, nchains, io, 0);
      default: return launch_loglik(m, w, nchains);
    }
  };
  struct Ev { hipEvent_t e0 = nullptr, e1 = nullptr; ~Ev() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); } } ev;   // destroyed on every return
  HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
  for (int i = 0; i < 3; ++i) if ((rc = launch_gene(m, w, nchains)) != PPCX_OK) return rc;
  HIPCHK(hipEventRecord(ev.e0, st));
  for (int i = 0; i < reps; ++i) if ((rc = one()) != PPCX_OK) return rc;
  HIPCHK(hipEventRecord(ev.e1, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_per_launch = (double)ms / reps;
#ifdef PPCX_TRACE
  if (const char* path = getenv("PPCX_TRACE_FILE")) {       // one more launch, stamped; the stamps go to the file as raw uint64
    const size_t n = (size_t)kTraceBlocks * 4 * kTracePasses * kTraceStamps;
    HIPCHK(hipMalloc(&g_trace_dev, sizeof(unsigned long long) * n));
    HIPCHK(hipMemset(g_trace_dev, 0, sizeof(unsigned long long) * n));
    rc = one();
    HIPCHK(hipStreamSynchronize(st));
    std::vector<unsigned long long> h(n);
    HIPCHK(hipMemcpy(h.data(), g_trace_dev, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    (void)hipFree(g_trace_dev); g_trace_dev = nullptr;
    if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), sizeof(unsigned long long), n, f); fclose(f); }
    if (rc != PPCX_OK) return rc;
  }
#endif
  return PPCX_OK;
}
#endif
