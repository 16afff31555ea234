// ppcx_fit_nuts.hip -- the NUTS fits: the direct-exchange group of a gene-sharded run (ppcx_xchg), what the four entry points
// share, the fit of chain groups on their own streams (fit_nuts_impl), the fit over gene shards (fit_sharded), the chains dealt
// to several devices and the one-call entry behind the R shim (ppcx_do_inference_C).
#include <string.h>
#include <chrono>
#include <thread>
#include "ppcx_host.h"

// ---- direct exchange between the ranks of a gene-sharded run (ppcx_kernels.h XchgArgs) ---------------------------------
struct ppcx_xchg {
  int device = 0, nranks = 1, rank = 0, max_chains = 0;
  void* local = nullptr; size_t bytes = 0;       // this rank's receive buffer: sums, then sequence numbers and abort words
  void* peer[kMaxRanks] = {};                    // every rank's buffer as this process sees it (peer[rank] = local)
  bool opened[kMaxRanks] = {};                   // mapped through an IPC handle (to be closed)
  bool connected = false;
  unsigned epoch = 0;                            // fits run over this group
  double timeout_s = 20.0;
  std::mutex* mu = nullptr;
};
static size_t xchg_bytes(int nranks, int max_chains) { return sizeof(double) * xchg_recv_doubles(nranks, max_chains) + sizeof(unsigned long long) * xchg_flag_words(nranks, max_chains); }
extern "C" int ppcx_xchg_create(int device, int nranks, int rank, int max_chains, ppcx_xchg** out) {
  if (!out || nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks || max_chains < 1 || max_chains > 1024)
    return fail(PPCX_ERR_ARG, "need 1 <= nranks <= 16, 0 <= rank < nranks, 1 <= max_chains <= 1024");
  *out = nullptr;
  HIPCHK(hipSetDevice(device));
  ppcx_xchg* x = new ppcx_xchg();
  x->device = device; x->nranks = nranks; x->rank = rank; x->max_chains = max_chains; x->bytes = xchg_bytes(nranks, max_chains);
  // uncached device memory: a peer's stores must be seen by loads of a kernel that is already running
  hipError_t e = hipExtMallocWithFlags(&x->local, x->bytes, hipDeviceMallocUncached);
  if (e == hipSuccess) e = hipMemset(x->local, 0, x->bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { ppcx_xchg_destroy(x); return fail(PPCX_ERR_HIP, std::string("exchange buffer: ") + hipGetErrorString(e)); }
  x->peer[rank] = x->local;
  if (nranks == 1) x->connected = true;
  *out = x;
  return PPCX_OK;
}
extern "C" int ppcx_xchg_handle(ppcx_xchg* x, char* out64) {
  if (!x || !out64) return fail(PPCX_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(x->device));
  hipIpcMemHandle_t h;
  HIPCHK(hipIpcGetMemHandle(&h, x->local));
  static_assert(sizeof(h) == 64, "hipIpcMemHandle_t is 64 bytes");
  memcpy(out64, &h, 64);
  return PPCX_OK;
}
extern "C" int ppcx_xchg_connect(ppcx_xchg* x, const char* handles) {
  if (!x || !handles) return fail(PPCX_ERR_ARG, "NULL argument");
  if (x->connected) return fail(PPCX_ERR_ARG, "the exchange group is connected already");
  HIPCHK(hipSetDevice(x->device));
  for (int k = 0; k < x->nranks; ++k) {
    if (k == x->rank) continue;
    hipIpcMemHandle_t h; memcpy(&h, handles + (size_t)k * 64, 64);
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(PPCX_ERR_HIP, "hipIpcOpenMemHandle (rank " + std::to_string(k) + "): " + hipGetErrorString(e));
    x->peer[k] = p; x->opened[k] = true;
  }
  x->connected = true;
  return PPCX_OK;
}
// ranks that live in ONE process (host threads, a shard model each -- on one device or several): plain device pointers
extern "C" int ppcx_xchg_connect_local(ppcx_xchg** group, int n) {
  if (!group || n < 1 || n > kMaxRanks) return fail(PPCX_ERR_ARG, "bad group");
  for (int k = 0; k < n; ++k) if (!group[k] || group[k]->nranks != n || group[k]->rank != k || group[k]->connected || group[k]->max_chains != group[0]->max_chains)
    return fail(PPCX_ERR_ARG, "group[k] must be the unconnected rank k of n, all with the same max_chains");
  for (int k = 0; k < n; ++k) {
    for (int j = 0; j < n; ++j) {
      if (group[k]->device != group[j]->device) {
        (void)hipSetDevice(group[k]->device);
        hipError_t e = hipDeviceEnablePeerAccess(group[j]->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(PPCX_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        (void)hipGetLastError();
      }
      group[k]->peer[j] = group[j]->local;
    }
    group[k]->connected = true;
  }
  return PPCX_OK;
}
extern "C" int ppcx_xchg_set_timeout(ppcx_xchg* x, double seconds) {
  if (!x || !(seconds > 0)) return fail(PPCX_ERR_ARG, "bad arguments");
  x->timeout_s = seconds;
  return PPCX_OK;
}
extern "C" void ppcx_xchg_destroy(ppcx_xchg* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  for (int k = 0; k < x->nranks; ++k) if (x->opened[k] && x->peer[k]) (void)hipIpcCloseMemHandle(x->peer[k]);
  (void)hipFree(x->local);
  delete x;
}
static void xchg_fill(const ppcx_xchg* x, XchgArgs* a) {
  a->nranks = x->nranks; a->rank = x->rank; a->max_chains = x->max_chains; a->chain0 = 0; a->epoch = x->epoch;
  a->timeout_ticks = (long long)(x->timeout_s * 1e8);
  const size_t nd = xchg_recv_doubles(x->nranks, x->max_chains);
  for (int k = 0; k < kMaxRanks; ++k) {
    a->recv[k] = k < x->nranks ? (double*)x->peer[k] : nullptr;
    a->flags[k] = k < x->nranks ? (unsigned long long*)((double*)x->peer[k] + nd) : nullptr;
  }
}

extern "C" void ppcx_nuts_config_default(ppcx_nuts_config* c) {
  if (!c) return;
  c->chains = 3; c->iter = 300; c->warmup = 150; c->seed = 1; c->adapt_delta = 0.8; c->max_treedepth = 10;
  c->init_radius = 2.0; c->stepsize0 = 1.0; c->init_buffer = 75; c->term_buffer = 50; c->window = 25;
  c->chain_id_offset = 0;
}
// ---- what the NUTS entry points share (fit_nuts_impl: ppcx_fit_nuts, ppcx_fit_nuts_xchg; fit_sharded: ppcx_fit_nuts_shards,
// ---- ppcx_fit_nuts_comm) -------------------------------------------------------------------------------------------------
static int nuts_config_check(const ppcx_nuts_config* cfg) {
  if (cfg->chains < 1 || cfg->chains > 1024 || cfg->iter < 1 || cfg->warmup < 0 || cfg->warmup > cfg->iter)
    return fail(PPCX_ERR_ARG, "need 1<=chains<=1024, iter>=1, 0<=warmup<=iter");
  if (cfg->max_treedepth < 1 || cfg->max_treedepth > kMaxDepth) return fail(PPCX_ERR_LIMIT, "max_treedepth must be in 1..10");
  return PPCX_OK;
}
static NutsConfig nuts_config(const ppcx_nuts_config* cfg) {
  NutsConfig nc;
  nc.chains = cfg->chains; nc.iter = cfg->iter; nc.warmup = cfg->warmup; nc.seed = cfg->seed; nc.adapt_delta = cfg->adapt_delta;
  nc.max_treedepth = cfg->max_treedepth; nc.init_radius = cfg->init_radius; nc.stepsize0 = cfg->stepsize0;
  nc.init_buffer = cfg->init_buffer; nc.term_buffer = cfg->term_buffer; nc.window = cfg->window;
  nc.chain_id_offset = cfg->chain_id_offset;
  return nc;
}
// A fit of `m` for the run `nc`, its buffers zero-filled on `st`, which is idle again on return: the chain groups of a fit run on
// streams of their own that nothing else orders against this one. A failure leaves nothing behind.
static int fit_create(ppcx_model* m, const NutsConfig& nc, hipStream_t st, ppcx_fit** out) {
  ppcx_fit* f = new ppcx_fit();
  fit_attach(f, m); f->chains = nc.chains; f->n_keep = nc.iter - nc.warmup; f->iter = nc.iter; f->cfg = nc;
  const size_t ni = (size_t)nc.chains * nc.iter, nk = (size_t)nc.chains * f->n_keep;
  hipError_t e = hipSuccess;
  if (nk > 0) e = f->d_draws.alloc_zeroed(nk * m->d.D, st);
  if (nk > 0 && e == hipSuccess) e = f->d_lp.alloc_zeroed(nk, st);
  if (e == hipSuccess) e = f->d_stepsize.alloc_zeroed(ni, st);
  if (e == hipSuccess) e = f->d_accept.alloc_zeroed(ni, st);
  if (e == hipSuccess) e = f->d_treedepth.alloc_zeroed(ni, st);
  if (e == hipSuccess) e = f->d_nleap.alloc_zeroed(ni, st);
  if (e == hipSuccess) e = f->d_div.alloc_zeroed(ni, st);
  if ((e = finish(e, st)) != hipSuccess) { ppcx_fit_free(f); return hip_fail(e, "the fit's buffers"); }
  *out = f;
  return PPCX_OK;
}
// where a run of the fit's chains from c0 on writes
static RunIO fit_io(const ppcx_fit* f, int c0) {
  const size_t k0 = (size_t)c0 * f->n_keep, i0 = (size_t)c0 * f->iter;
  const long D = f->m->d.D;
  RunIO io;
  io.draws = f->d_draws.p ? f->d_draws.p + k0 * D : nullptr; io.draws_stride = (long)f->n_keep * D;
  io.n_keep = f->n_keep; io.iter = f->iter;
  io.lp = f->d_lp.p ? f->d_lp.p + k0 : nullptr;
  io.stepsize = f->d_stepsize.p + i0; io.accept = f->d_accept.p + i0;
  io.treedepth = f->d_treedepth.p + i0; io.nleap = f->d_nleap.p + i0; io.div = f->d_div.p + i0;
  return io;
}
// the initial states of the chains c0 .. c0 + n - 1 of the run `nc` into w, a Work of n chains
static int upload_initial_states(Work& w, const NutsConfig& nc, int c0, int n) {
  std::vector<ChainState> states(n);
  NutsConfig ncg = nc; ncg.chain_id_offset = nc.chain_id_offset + c0;
  for (int c = 0; c < n; ++c) state_init(states[c], ncg, c, 0);
  HIPCHK(hipMemcpyAsync(w.states[0].p, states.data(), sizeof(ChainState) * n, hipMemcpyHostToDevice, w.stream));
  HIPCHK(hipStreamSynchronize(w.stream));       // `states` is a host temporary
  return PPCX_OK;
}
// the launch budget of a run's pump: a round per leapfrog of the deepest trees and some more; a pipelined round counts twice
static long long max_pairs(const ppcx_nuts_config* cfg, int per_round) {
  return ((long long)cfg->iter * ((1LL << cfg->max_treedepth) + 8) + 100000) * per_round;
}
static void fit_record(ppcx_fit* f, const PumpStats& ps, double seconds, long long leapfrogs) {
  f->seconds = seconds;
  f->grad_evals = leapfrogs;
  f->kA_samples = ps.kA_samples;
  f->kA_ms_mean = ps.kA_samples ? ps.kA_ms_sum / (double)ps.kA_samples : 0.0;
  f->kA_chain_launches_mean = ps.kA_samples ? ps.chain_launches / (double)ps.kA_samples : 0.0;
  f->kC_ms_mean = ps.kA_samples ? ps.kC_ms_sum / (double)ps.kA_samples : 0.0;
  f->kU_ms_mean = ps.kA_samples ? ps.kU_ms_sum / (double)ps.kA_samples : 0.0;
  f->launch_triples = ps.pairs;
}

#ifdef PPCX_TESTING
static std::mutex g_sm_mutex; static long long g_sm_ticks[6] = {0, 0, 0, 0, 0, 0}; static long long g_sm_rounds = 0;
// mean microseconds per round a chain's state machine (the workgroup beside the log-likelihood workgroups of a pipelined round)
// spent in its phases, over the fits since the last call: [0] until state, command, hyper vectors and slab have arrived,
// [1] folding the slab and staging in LDS, [2] the exchange between ranks, [3] chain_step, [4] after it; out[5] = rounds counted
extern "C" int ppcx_testing_sm_trace(double* out6) {
  std::lock_guard<std::mutex> lk(g_sm_mutex);
  for (int k = 0; k < 5; ++k) out6[k] = g_sm_rounds ? 1e-2 * (double)g_sm_ticks[k] / (double)g_sm_rounds : 0.0;
  out6[5] = (double)g_sm_rounds;
  for (int k = 0; k < 6; ++k) g_sm_ticks[k] = 0;
  g_sm_rounds = 0;
  return PPCX_OK;
}
#endif
static int fit_nuts_impl(ppcx_model* m, const ppcx_nuts_config* cfg, ppcx_xchg* xg, ppcx_fit** out) {
  if (!m || !cfg || !out) return fail(PPCX_ERR_ARG, "NULL argument");
  *out = nullptr;
  int rc = nuts_config_check(cfg);
  if (rc != PPCX_OK) return rc;
  HIPCHK(hipSetDevice(m->device));
  const int nch = cfg->chains, D = m->d.D;
  choose_launch(m, (xg && xg->nranks > 1) ? nch : fit_launch_chains(m, nch));   // (between ranks: one group, below)
  // Round structure. Pipelined (default where it applies): two launches per leapfrog, the state machine beside the
  // log-likelihood workgroups (ppcx_kernels_ls.hip, "Pipelined rounds"). It needs a model whose cells read the anticipated
  // constants only (no per-cell linear predictor). The choice must not depend on the number of chains: the two round
  // structures sum the kinetic energy of fresh momenta in different orders, and a chain's draws may not depend on its
  // company. (With more chains than the chip holds workgroups the state machines simply run ahead of the log-likelihood
  // workgroups instead of beside them.) ppcx_model_set_rounds(m, 0, ...) selects the three-launch round.
  const bool piped = model_pipelines(m);
  // The exchange group is looked at BEFORE anything is allocated (a refused call leaves nothing behind), and the group's fit
  // counter -- the epoch in every sequence number -- moves before anything that can fail on one rank alone: a rank whose
  // allocation fails has then counted this fit like its peers, and it tells them that it has left (leave() below) instead of
  // letting them wait for the timeout, now and in every later fit of the group.
  XchgArgs xa;
  bool xa_live = false;
  if (xg) {
    if (!xg->connected) return fail(PPCX_ERR_ARG, "the exchange group is not connected");
    if (xg->device != m->device) return fail(PPCX_ERR_ARG, "the exchange group lives on another device than the shard");
    if (cfg->chains > xg->max_chains) return fail(PPCX_ERR_ARG, "more chains than the exchange group was created for");
    if (!piped) return fail(PPCX_ERR_LIMIT, "the direct exchange runs inside pipelined rounds, which ppcx_model_set_rounds (or a model too large for "
                                             "the merged launch's LDS) rules out: use ppcx_fit_nuts_comm");
    xg->epoch += 1;                             // every rank counts the fits of the group: sequence numbers of earlier fits never match
    xchg_fill(xg, &xa);
    xa_live = xg->nranks > 1;
  }
  ppcx_fit* f = nullptr;
  auto leave = [&](int rc) {                    // every failure from here on: the peers' state machines are told, the fit is freed
    const std::string msg = g_err;
    if (xa_live) { (void)launch_xchg_abort_kernel(xa, m->stream.s); (void)hipStreamSynchronize(m->stream.s); }
    if (f) ppcx_fit_free(f);
    g_err = msg;
    return rc;
  };
  const NutsConfig nc = nuts_config(cfg);
  if ((rc = fit_create(m, nc, m->stream.s, &f)) != PPCX_OK) return leave(rc);
  f->inv_metric.assign((size_t)nch * D, 1.0);
  // Chains can also be split into groups that run on their own streams from their own host threads
  // (ppcx_model_set_rounds): while one group sits in its memory-bound gene kernel another group's log-likelihood
  // workgroups have the CUs: measured at cfg3 / 8 chains, pipelined rounds (final kernels of round 3, mean of two fits):
  // 3.13 s per fit on one stream, 2.97 s with two groups, 2.93 s with three. Default: three groups from eight chains on, two
  // from four (whole fits at cfg3 size, one group -> two: 4 chains 2.00 -> 1.82 s, 5 chains 2.40 -> 2.07, 6 chains
  // 2.86 -> 2.37, 7 chains 3.21 -> 2.64; three chains are faster on one stream; four groups are slower everywhere). A chain's draws do not depend on the grouping (tests/test_gpu_configs.py); the per-kernel event timings of a
  // fit are only meaningful with one group (bench.py takes its roofline sample from a fit on one stream).
  int ngrp = fit_stream_groups(m, nch);
  // Between ranks (direct exchange) the chains run as ONE group on one stream: a chain's state machine spins inside its merged
  // launch until every peer's copy of that chain has published its sums, so the peers' launches of the SAME group must be running
  // at the same time. With several groups a rank's launch of group A can sit in front of its launch of group B while the peer
  // has them the other way round -- each state machine then waits for a launch that is queued behind the one it is waiting in,
  // until the exchange's timeout ends the fit.
  if (xa_live) ngrp = 1;
  struct Group { int c0 = 0, n = 0; Work w; RunIO io; PumpStats ps; int rc = PPCX_OK; std::string err; long long leap = 0, xticks = 0, xcount = 0; };
  std::vector<Group> grp(ngrp);
  std::atomic<int> stop{0};
  const long long budget = max_pairs(cfg, piped ? 2 : 1);
  for (int g = 0; g < ngrp; ++g) {
    Group& G = grp[g];
    G.w.pipelined = piped;
    G.c0 = (int)((long long)nch * g / ngrp); G.n = (int)((long long)nch * (g + 1) / ngrp) - G.c0;
    G.w.xchg_chain0 = G.c0;                    // also what a progress report names the group by
    G.w.stop = &stop;
    G.w.shared_chip = ngrp > 1;
    if (xg && xg->nranks > 1) G.w.xchg = &xa;
    if (g > 0) {
      const hipError_t e = G.w.own.create();
      if (e != hipSuccess) return leave(hip_fail(e, "hipStreamCreateWithFlags (chain group)"));
      G.w.stream = G.w.own.s;
    }
    if ((rc = work_alloc(G.w, m, G.n)) != PPCX_OK) return leave(rc);
    if ((rc = upload_initial_states(G.w, nc, G.c0, G.n)) != PPCX_OK) return leave(rc);
    G.io = fit_io(f, G.c0);
  }
  const auto t0 = std::chrono::steady_clock::now();
  auto run_group = [&](Group* G) {
    (void)hipSetDevice(m->device);
    G->rc = pump(m, G->w, G->n, G->io, budget, true, &G->ps);
    if (G->rc != PPCX_OK) { G->err = g_err; return; }
    std::vector<ChainState> states(G->n);
    if (hipMemcpy(states.data(), current_states(G->w), sizeof(ChainState) * G->n, hipMemcpyDeviceToHost) != hipSuccess) {
      G->rc = PPCX_ERR_HIP; G->err = "reading back the chain states failed"; return;
    }
    for (int c = 0; c < G->n; ++c) { G->leap += states[c].sc.total_leapfrogs; G->xticks += states[c].xc.ticks; G->xcount += states[c].xc.count; }
#ifdef PPCX_TESTING
    { std::lock_guard<std::mutex> lk(g_sm_mutex); for (int c = 0; c < G->n; ++c) { for (int k = 0; k < 6; ++k) g_sm_ticks[k] += states[c].tr.t[k]; g_sm_rounds += states[c].tr.n; } }
#endif
    // the adapted inverse metric (what rstan::get_adaptation_info prints): the genes' coordinates, then the six hyper-parameters
    std::vector<double> hq((size_t)G->n * V_COUNT * 8);
    bool ok = hipMemcpy(hq.data(), current_hyper(G->w), sizeof(double) * hq.size(), hipMemcpyDeviceToHost) == hipSuccess;
    for (int c = 0; c < G->n && ok; ++c) {
      double* dst = f->inv_metric.data() + (size_t)(G->c0 + c) * D;
      ok = hipMemcpy(dst, G->w.vecs.p + ((size_t)c * V_COUNT + V_MINV) * G->w.Dpad, sizeof(double) * D, hipMemcpyDeviceToHost) == hipSuccess;
      for (int k = 0; k < 6; ++k) dst[hyper_index(m->d, k)] = hq[((size_t)c * V_COUNT + V_MINV) * 8 + k];
    }
    if (!ok) { G->rc = PPCX_ERR_HIP; G->err = "reading back the inverse metric failed"; }
  };
  {
    std::vector<std::thread> th;
    for (int g = 1; g < ngrp; ++g) th.emplace_back(run_group, &grp[g]);
    run_group(&grp[0]);
    for (auto& t : th) t.join();
  }
  const auto t1 = std::chrono::steady_clock::now();
  for (int g = 0; g < ngrp; ++g) if (grp[g].rc != PPCX_OK) {
    const int rc = grp[g].rc; const std::string e = grp[g].err;
    return leave(fail(rc, e));                   // (the peers' state machines wait for this rank: leave() tells them it has left)
  }
  PumpStats ps;
  long long leap = 0;
  for (int g = 0; g < ngrp; ++g) {
    leap += grp[g].leap; f->xchg_ticks += grp[g].xticks; f->xchg_count += grp[g].xcount;
    ps.kA_ms_sum += grp[g].ps.kA_ms_sum; ps.kC_ms_sum += grp[g].ps.kC_ms_sum; ps.kU_ms_sum += grp[g].ps.kU_ms_sum;
    ps.kA_samples += grp[g].ps.kA_samples; ps.chain_launches += grp[g].ps.chain_launches; ps.pairs += grp[g].ps.pairs;
  }
  fit_record(f, ps, std::chrono::duration<double>(t1 - t0).count(), leap);
  *out = f;
  return PPCX_OK;
}
extern "C" int ppcx_fit_nuts(ppcx_model* m, const ppcx_nuts_config* cfg, ppcx_fit** out) { return fit_nuts_impl(m, cfg, nullptr, out); }
// One gene shard per rank, the ranks' sums added by the state machines themselves (direct exchange): the pipelined round of
// ppcx_fit_nuts with one more step inside the merged launch. Every rank calls it with the same configuration.
extern "C" int ppcx_fit_nuts_xchg(ppcx_model* shard, const ppcx_nuts_config* cfg, ppcx_xchg* xg, ppcx_fit** out) {
  if (!xg) return fail(PPCX_ERR_ARG, "exchange group is NULL");
  return fit_nuts_impl(shard, cfg, xg, out);
}

static int fit_sharded(ppcx_model** models, int ns, const ppcx_nuts_config* cfg, ppcx_comm* comm, ppcx_fit** fits) {
  if (!models || !cfg || !fits || ns < 1 || ns > kMaxShards) return fail(PPCX_ERR_ARG, "bad shard arguments");
  for (int k = 0; k < ns; ++k) { fits[k] = nullptr; if (!models[k]) return fail(PPCX_ERR_ARG, "NULL shard model"); }
  int rc = nuts_config_check(cfg);
  if (rc != PPCX_OK) return rc;
  const int dev = models[0]->device;
  for (int k = 0; k < ns; ++k) if (models[k]->device != dev) return fail(PPCX_ERR_ARG, "in-process shards must share a device");
  HIPCHK(hipSetDevice(dev));
  const int nch = cfg->chains;
  const NutsConfig nc = nuts_config(cfg);
  hipStream_t st = models[0]->stream.s;           // all in-process shards are ordered on one stream
  std::vector<Work> works(ns);
  std::vector<Shard> sh(ns);
  auto drop = [&](int code) { for (int k = 0; k < ns; ++k) { ppcx_fit_free(fits[k]); fits[k] = nullptr; } return code; };   // (g_err stays)
  for (int k = 0; k < ns; ++k) {
    ppcx_model* m = models[k];
    choose_launch(m, nch);
    if ((rc = fit_create(m, nc, st, &fits[k])) != PPCX_OK) return drop(rc);
    works[k].stream = st;
    if ((rc = work_alloc(works[k], m, nch)) != PPCX_OK) return drop(rc);
    if ((rc = upload_initial_states(works[k], nc, 0, nch)) != PPCX_OK) return drop(rc);   // every shard replicates the same chains
    sh[k].m = m; sh[k].w = &works[k]; sh[k].io = fit_io(fits[k], 0);
  }
  PumpStats ps;
  const auto t0 = std::chrono::steady_clock::now();
  rc = pump(sh, nch, comm, max_pairs(cfg, 1), true, &ps);
  const auto t1 = std::chrono::steady_clock::now();
  if (rc != PPCX_OK) return drop(rc);
  std::vector<ChainState> states(nch);
  const hipError_t e = hipMemcpy(states.data(), current_states(works[0]), sizeof(ChainState) * nch, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return drop(hip_fail(e, "reading back the chain states"));
  long long leap = 0;
  for (int c = 0; c < nch; ++c) leap += states[c].sc.total_leapfrogs;
  // (no adapted metric and no exchange timing on these fits: ppcx_fit_get_inv_metric refuses them)
  for (int k = 0; k < ns; ++k) fit_record(fits[k], ps, std::chrono::duration<double>(t1 - t0).count(), leap);
  return PPCX_OK;
}
extern "C" int ppcx_fit_nuts_shards(ppcx_model** models, int n_shards, const ppcx_nuts_config* cfg, ppcx_fit** fits) {
  return fit_sharded(models, n_shards, cfg, nullptr, fits);
}
extern "C" int ppcx_fit_nuts_comm(ppcx_model* shard, const ppcx_nuts_config* cfg, ppcx_comm* comm, ppcx_fit** out) {
  if (!comm) return fail(PPCX_ERR_ARG, "communicator is NULL");
  return fit_sharded(&shard, 1, cfg, comm, out);
}

// One NUTS pass with the CHAINS dealt to several devices of this process -- what rstan::sampling(chains, cores) does with its
// worker processes (R/utilities.R:1497-1512, :1377-1386) -- behind the .C() entry: one host thread per device creates the model
// there, runs its share of the chains (global chain ids: the chains' Philox streams do not depend on the device they run on) and
// hands back the checked genes' columns of its kept draws; the first device then holds a model of the K checked genes and computes
// the generated quantities from the pooled chains, as rstan::summary does over merged chains (:685-703). Lanes per gene are those a
// single device would choose for ALL the chains, so the result does not depend on the number of devices.
static int nuts_over_devices(const int* devs, int ndev, int G, int S, int C, int K, const int* counts, const double* X, const double* exposure,
                             double lmm, int n_excl, const int* excl, const ppcx_nuts_config& cfg0, double tc, double p_lo, double p_hi,
                             unsigned long long seed, int n_gen, int resample, double* ci, double* slope, int* counts_rng) {
  const int chains = cfg0.chains, n_keep = cfg0.iter - cfg0.warmup;
  if (n_keep < 1) return fail(PPCX_ERR_ARG, "no kept draws");
  if (ndev > chains) ndev = chains;
  const int per = (chains + ndev - 1) / ndev;
  const int n2 = C > 2 ? C - 2 : 0, nsl = C - 1 > 1 ? C - 1 : 1;
  const int Dk = 2 * K + K * nsl + 6;
  std::vector<double> pooled((size_t)chains * n_keep * Dk, 0.0);
  std::vector<int> rcs(ndev, PPCX_OK); std::vector<std::string> errs(ndev);
  auto work = [&](int r) {
    const int c0 = r * per, n = chains - c0 < per ? chains - c0 : per;
    if (n <= 0) return;
    ppcx_model* m = nullptr; ppcx_fit* f = nullptr;
    int rc = ppcx_model_create(devs[r], G, S, C, K, counts, X, exposure, lmm, n_excl, excl, &m);
    if (rc == PPCX_OK) {
      choose_launch(m, fit_launch_chains(m, chains));   // the geometry of ONE fit of all the chains
      m->L_override = m->L;
      ppcx_nuts_config cfg = cfg0; cfg.chains = n; cfg.chain_id_offset = cfg0.chain_id_offset + c0;
      rc = ppcx_fit_nuts(m, &cfg, &f);
    }
    if (rc == PPCX_OK) {
      const Dims& d = m->d;
      std::vector<int32_t> cols;
      for (int k = 0; k < 3; ++k) cols.push_back(k);
      for (int k = 0; k < K; ++k) cols.push_back(d.off_intercept + k);
      for (int k = 0; k < K; ++k) cols.push_back(d.off_alpha1 + k);
      for (int k = 0; k < n2 * K; ++k) cols.push_back(d.off_alpha2 + k);
      for (int k = 0; k < K; ++k) cols.push_back(d.off_sigma_raw + k);
      for (int k = 0; k < 3; ++k) cols.push_back(d.off_tail + k);
      rc = (int)cols.size() == Dk ? ppcx_fit_get_columns(f, Dk, cols.data(), pooled.data() + (size_t)c0 * n_keep * Dk)
                                  : fail(PPCX_ERR_ARG, "checked columns do not match the K-gene model");
    }
    if (rc != PPCX_OK) errs[r] = g_err;          // (g_err is per thread)
    rcs[r] = rc;
    ppcx_fit_free(f); ppcx_model_destroy(m);
  };
  {
    std::vector<std::thread> th;
    for (int r = 1; r < ndev; ++r) th.emplace_back(work, r);
    work(0);
    for (auto& t : th) t.join();
  }
  for (int r = 0; r < ndev; ++r) if (rcs[r] != PPCX_OK) return fail(rcs[r], "device " + std::to_string(devs[r]) + ": " + errs[r]);
  // the K checked genes on the first device: cell ids g * S + s and draw indices are those of the full model
  std::vector<int> ex_k;
  for (int e = 0; e < n_excl; ++e) if (excl[e] / S < K) ex_k.push_back(excl[e]);
  ppcx_model* mk = nullptr; ppcx_fit* fk = nullptr;
  int rc = ppcx_model_create(devs[0], K, S, C, K, counts, X, exposure, lmm, (int)ex_k.size(), ex_k.data(), &mk);
  if (rc == PPCX_OK) rc = ppcx_fit_from_draws(mk, chains, n_keep, pooled.data(), &fk);
  if (rc == PPCX_OK) rc = ppcx_fit_ppc(fk, tc, p_lo, p_hi, seed, n_gen, resample, ci, counts_rng);
  if (rc == PPCX_OK && slope) {
    for (int k = 0; k < K; ++k) {
      double s = 0;
      for (long r = 0; r < (long)chains * n_keep; ++r) s += pooled[(size_t)r * Dk + 3 + K + k];
      slope[k] = s / ((double)chains * n_keep);
    }
  }
  ppcx_fit_free(fk); ppcx_model_destroy(mk);
  return rc;
}

extern "C" void ppcx_do_inference_C(const int* dims, const int* counts, const double* X, const double* exposure,
                                    const int* excl, const double* reals, double* ci, double* slope, int* counts_rng,
                                    int* status, char** errbuf, const int* errlen) {
  if (!status) return;
  auto finish = [&](int rc) {
    *status = rc;
    if (errbuf && errbuf[0] && errlen && errlen[0] > 0) {
      const char* msg = rc == PPCX_OK ? "" : g_err.c_str();
      strncpy(errbuf[0], msg, (size_t)errlen[0] - 1);
      errbuf[0][errlen[0] - 1] = 0;
    }
  };
  if (!dims || !reals || !ci) { finish(fail(PPCX_ERR_ARG, "dims, reals and ci must not be NULL")); return; }
  if (dims[0] != PPCX_VERSION) {               // a shim written for another argument layout: nothing else is read
    finish(fail(PPCX_ERR_ARG, "ppcx_do_inference_C: dims[0] must be the ABI version the caller was written for (" + std::to_string(PPCX_VERSION) + "), got " + std::to_string(dims[0])));
    return;
  }
  dims += 1;                                   // the fields below are numbered as in include/ppcx.h, after the version
  const int device = dims[0], G = dims[1], S = dims[2], C = dims[3], K = dims[4], n_excl = dims[5];
  const int vb = dims[11], save_rng = dims[12];
  if (save_rng && !counts_rng) { finish(fail(PPCX_ERR_ARG, "save_generated_quantities without a counts_rng buffer")); return; }
  const int n_devices = dims[15];
  if (n_devices < 0 || n_devices > 16) { finish(fail(PPCX_ERR_ARG, "n_devices must be 0 .. 16")); return; }
  if (!vb && n_devices > 1 && K > 0) {          // the chains over several devices (ADVI is one chain: the first device)
    ppcx_nuts_config cfg; ppcx_nuts_config_default(&cfg);
    cfg.chains = dims[6]; cfg.iter = dims[7]; cfg.warmup = dims[8]; cfg.seed = (unsigned long long)reals[4];
    finish(nuts_over_devices(dims + 16, n_devices, G, S, C, K, counts, X, exposure, reals[0], n_excl, excl, cfg, reals[1], reals[2], reals[3],
                             (unsigned long long)reals[4], dims[9], dims[10], ci, slope, save_rng ? counts_rng : nullptr));
    return;
  }
  ppcx_model* m = nullptr; ppcx_fit* f = nullptr;
  int rc = ppcx_model_create(n_devices >= 1 ? dims[16] : device, G, S, C, K, counts, X, exposure, reals[0], n_excl, excl, &m);
  if (rc == PPCX_OK) {
    if (vb) {
      ppcx_advi_config ac; ppcx_advi_config_default(&ac);
      ac.output_samples = dims[13]; ac.iter = dims[14] > 0 ? dims[14] : 50000; ac.seed = (unsigned long long)reals[4];
      if (reals[5] > 0) ac.tol_rel_obj = reals[5];
      rc = ppcx_fit_advi_iterative(m, &ac, 5, &f);
    } else {
      ppcx_nuts_config cfg; ppcx_nuts_config_default(&cfg);
      cfg.chains = dims[6]; cfg.iter = dims[7]; cfg.warmup = dims[8]; cfg.seed = (unsigned long long)reals[4];
      rc = ppcx_fit_nuts(m, &cfg, &f);
    }
  }
  if (rc == PPCX_OK) rc = ppcx_fit_ppc(f, reals[1], reals[2], reals[3], (unsigned long long)reals[4], dims[9], dims[10], ci,
                                       save_rng ? counts_rng : nullptr);
  if (rc == PPCX_OK && slope && K > 0) {
    std::vector<int32_t> cols(K);
    for (int k = 0; k < K; ++k) cols[k] = m->d.off_alpha1 + k;
    int chains, n_keep; ppcx_fit_info(f, &chains, &n_keep, nullptr, nullptr);
    std::vector<double> a((size_t)chains * n_keep * K);
    rc = ppcx_fit_get_columns(f, K, cols.data(), a.data());
    if (rc == PPCX_OK) for (int k = 0; k < K; ++k) {
      double s = 0; for (long r = 0; r < (long)chains * n_keep; ++r) s += a[(size_t)r * K + k];
      slope[k] = s / ((double)chains * n_keep);
    }
  }
  ppcx_fit_free(f); ppcx_model_destroy(m);
  finish(rc);
}
