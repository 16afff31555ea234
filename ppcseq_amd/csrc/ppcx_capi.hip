// ppcx_capi.hip -- host side of the C ABI declared in include/ppcx.h, first part: the error state, the model (creation, gene
// shards, setters and getters) and the launch geometry. The others: ppcx_run.hip (a run's scratch, its launches, the pump, the
// RCCL binding), ppcx_fit_nuts.hip, ppcx_fit_advi.hip (the fits) and ppcx_fit_api.hip (what is read from a fit). ppcx_host.h
// states what they share. No torch types, no exceptions across the boundary.
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <memory>
#include "ppcx_host.h"

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int hip_fail(hipError_t e, const char* what) { return fail(PPCX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
int hip_done(const char* who, hipError_t e) {
  return e == hipSuccess ? PPCX_OK : who ? hip_fail(e, who) : fail(PPCX_ERR_HIP, hipGetErrorString(e));
}
#ifdef PPCX_TESTING
TestHooks g_test;
#endif

extern "C" int ppcx_version(void) { return PPCX_VERSION; }
extern "C" int ppcx_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
extern "C" const char* ppcx_last_error(void) { return g_err.c_str(); }
extern "C" int ppcx_device_memory(int device, unsigned long long* free_bytes, unsigned long long* total_bytes) {
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PPCX_ERR_ARG, "no such HIP device");
  HIPCHK(hipSetDevice(device));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (unsigned long long)f;
  if (total_bytes) *total_bytes = (unsigned long long)t;
  return PPCX_OK;
}

// Launch geometry of the log-likelihood kernel. The launch is resident: n_res = (workgroups the chip holds at once)
// divided among the chains of the launch, four wavefronts each; wavefront j of a chain walks the gene positions
// bounds[j] .. bounds[j + 1] of the gene order, 64 / L genes per pass.
//   pass cost (in row-sweep iterations of a lane): 5.8 for loading and closing the genes -- 129 vector instructions against
//   43.7 per iteration (SQ_INSTS_VALU at S = 40, 104, 200) are 3 iterations' worth of issue, but with the dependent loads at
//   the start of a pass they weigh like 5 to 6 in time (L = 8 against 16 at 4 chains, 4 against 8 at 3 chains: measured), ceil(S / L) for the row sweep
//   (a little more on the two-group path, 2.5 x on the generic path with an exp per cell), 0.75 per iteration of the
//   low-count loop, which lasts as long as the longest list of the pass needs -- from the kernel's instruction counts
//   (profiles/, SQ_INSTS_VALU: ~50 per row-sweep cell, ~100 per list cell, ~250 per pass).
//   L: minimise passes x pass cost for the full chain count (chosen once per fit: a gene's sums depend on L).
//   bounds: contiguous ranges of whole passes of (nearly) equal cost -- the boundary of wavefront j is where the running
//   cost crosses j / (wavefronts per chain) of the total; recomputed when chains finish and the others get their slots.
// (A streamed model -- ppcx_model::streamed -- is planned by the same costs: nobody has measured what its passes cost relative to
// one another, and its sums depend on the lanes per gene only, as everyone's.)
static double pass_cost(const ppcx_model* m, int L, int p, int n) {
  const int S = m->d.S;
  bool slope = false;
  for (int i = p; i < p + n; ++i) slope = slope || m->pos_slope[i];
  // a pass of genes with slopes: 1.15 x a plain one in a two-group design. With more indicator columns it costs 1.43 x (C = 3, all
  // genes with slopes against none: 83.9 vs 58.4 us per launch) -- but weighting it so makes the launch SLOWER (K = 1000 of 20 000
  // genes: weight 1.0 -> 63.4 us, 1.45 -> 67.5, 2.0 -> 72.8; scripts/gpu_factor_k.py): the four wavefronts of a SIMD come from four
  // workgroups and share its fp64 unit, so what counts is the SIMD's total, and a wavefront with fewer, dearer passes does not
  // relieve the three it shares the SIMD with, while the passes it gives up push the others over their share
  double slope_w = m->d.C > 2 ? 1.0 : 1.15;
#ifdef PPCX_TESTING
  if (g_test.slope_cost_permille > 0) slope_w = 1e-3 * g_test.slope_cost_permille;
#endif
  // ... and with an exp per cell (a continuous covariate: sweep_cells MODE 3; without the column of ones: generic_cells)
  double lin_w = 2.5;
#ifdef PPCX_TESTING
  if (g_test.slope_cost_permille > 0) lin_w = 1e-3 * g_test.slope_cost_permille;
#endif
  const double sweep = (double)((S + L - 1) / L) * (!m->d.x0_is_one ? 2.5 : (slope && !m->d.x1_binary ? lin_w : (slope ? slope_w : 1.0)));
  return 5.8 + sweep;
}
// reserve: workgroups of the same launch that are not log-likelihood workgroups (the state machines of a pipelined
// round's merged launch; they are dispatched first and resident for a part of the launch)
static int resident_workgroups(const ppcx_model* m, int reserve) {
  int n = m->wgs_override > 0 ? m->wgs_override : m->n_cu * (reserve > 0 ? m->ls_wgs_per_cu : m->wgs_per_cu);
  n -= reserve;
  return n < 1 ? 1 : n;
}
// workgroups per chain: all of the resident ones, a multiple of 8 (the kernel deals runs of 8 to the XCDs), not more
// than there are passes to hand out
constexpr double kTrimSlack = 0.0;
static int workgroups_per_chain(const ppcx_model* m, int L, int nch, int n_res, bool whole_runs = true, bool trim = false) {
  int nbpc = n_res / (nch < 1 ? 1 : nch);
  if (nbpc >= 8 && whole_runs) nbpc = nbpc / 8 * 8;
  if (nbpc < 1) nbpc = 1;
  const int gpw = 64 / L, npass = (m->d.G + gpw - 1) / gpw;
  if (nbpc > (npass + 3) / 4) nbpc = (npass + 3) / 4;
  // trim (a launch of one of several chain groups, whose launches share the chip): ... and not more than it takes to give every
  // wavefront the passes of the busiest one. A launch lasts as long as its wavefront with the most passes (plan_launch); with
  // 2500 passes for 1352 wavefronts (cfg3, a chain group of three) that is two, for a sixth of the wavefronts one -- scattered
  // by the cost balancing, so that nearly every workgroup keeps its slot for the whole launch with a wavefront less to run.
  // 1250 wavefronts with two passes each last as long and leave 8 % of the chip's slots (39 % in a launch of two chains) to the
  // launch of another chain group, which otherwise waits for them: cfg3, 8 chains in three groups, 2.75 -> 2.53 s per fit
  // (round 4). No slack beyond the whole run of 8 workgroups pays (kTrimSlack: 0 / 1.5 / 3 / 6 / 12 % -> 2.55 / 2.55 / 2.58 / 2.62 /
  // 2.66 s), nor a pass more per wavefront on fewer workgroups (2.82 s). Alone on the chip the trimmed launch is the slower one
  // (nobody takes the slots, and the balancing has less to work with: 3 chains 27.9 -> 30.3 us, 8 chains on one stream
  // 2.95 -> 3.31 s per fit), so a fit on one stream keeps every resident workgroup.
  // A gene's sums depend on the lanes per gene only: the chains do not change.
  if (trim) {
    double slack = kTrimSlack;
#ifdef PPCX_TESTING
    if (g_test.trim_slack_permille >= 0) slack = 1e-3 * g_test.trim_slack_permille;
#endif
    int maxp = (npass + 4 * nbpc - 1) / (4 * nbpc);
#ifdef PPCX_TESTING
    maxp += g_test.trim_extra_passes;
#endif
    int nb2 = (int)ceil((double)npass * (1.0 + slack) / (4.0 * maxp));
    if (nb2 >= 8 && whole_runs) nb2 = (nb2 + 7) / 8 * 8;
    if (nb2 < nbpc) nbpc = nb2;
  }
  return nbpc;
}
// chain groups on their own streams (ppcx_fit_nuts): the default for a fit of `nch` chains, and what ppcx_model_set_rounds makes of it
static int default_stream_groups(int nch) { return nch >= 8 ? 3 : (nch >= 4 ? 2 : 1); }
// chains in a launch of a fit of `nch` chains: the fit runs them in groups on their own streams (ppcx_model_set_rounds, default
// default_stream_groups), every launch holds one group. A function of the fit's chain count and the model's setting only, so that a
// chain's lanes per gene -- hence its draws -- do not depend on anything else.
int fit_stream_groups(const ppcx_model* m, int nch) {
  if (m->opt_stream_groups >= 1) return m->opt_stream_groups < nch ? m->opt_stream_groups : nch;
  return default_stream_groups(nch);
}
int fit_launch_chains(const ppcx_model* m, int nch) {
  const int g = fit_stream_groups(m, nch);
  return (nch + g - 1) / g;
}
// the planned ranges go (on the model's device) where lanes per gene, the resident workgroups or the gene order change
static void drop_plans(ppcx_model* m) {
  std::lock_guard<std::mutex> lk(m->plan_mutex);
  m->plans.clear();
}
void choose_launch(ppcx_model* m, int nchains) {
  const int G = m->d.G, S = m->d.S;
  // lanes per gene for launches of `nchains` chains: passes of the busiest wavefront x pass cost, smallest first. A pass costs
  // what its sweep costs plus 8 cell iterations' worth of loading and closing its genes (round 5: SQ_INSTS_VALU of a wavefront
  // = 22 per cell iteration + 165 per pass; rounds 2-4, with a cell of 41 instructions: 5.8).
  // Round 5 dropped two things. (a) The condition that a choice leave no wavefront slot of the chip without a pass (>= 1.2 passes
  // per slot), which kept few large passes from looking cheapest at small numbers of chains: with the cheaper cell the pass
  // overhead decides, and the measured order is the model's -- cfg3, kernel level, one chain: L = 8 9.4 us (2500 wavefronts of one
  // pass), 4 10.9, 16 11.4, 32 13.5; two chains: L = 4 13.5, 8 15.9, 16 17.6, 32 20.5; three: L = 4 15.8, 8 17.6; eight: L = 8
  // 38.6, 4 39.0. (b) Choosing L for all the chains of a fit when the fit runs them in groups (callers pass the chains of a
  // group's launch, fit_launch_chains): whole cfg3 fits by L = 4 / 8 / 16 (scripts/gpu_lanes_fits.py): 1 chain 0.920 / 0.918 /
  // 0.950 s, 2 chains 1.008 / 1.081 / 1.114, 3 chains 1.152 / 1.272 / 1.495, 4 chains (two groups) 1.256 / 1.281 / 1.358, 8 chains
  // (three groups) 1.634 / 1.756 / 1.978. (Round 3 had measured the same 9 % at 8 chains and not taken them: two of 61 fits with
  // L = 4 ended warm-up with a chain at tree depth 10, none of 233 with L = 8. Round 5 found where such chains come from --
  // log(-sigma_slope) wandering through its flat tail during the one adaptation window, DESIGN.md section 4 -- and lanes per gene
  // have no part in it beyond changing every chain's rounding, like a seed.)
  int bestL = 64; double best = 1e300;
  for (int L = 64; L >= 1; L >>= 1) {                      // (ties go to the larger L: shorter dependent chains per lane)
    const int gpw = 64 / L;
    // (L = 1, 2: a lane's four counts of a trip lie 4 L bytes apart, every request touches 64 / L times the lines: +20 %)
    const double npass = ceil((double)G / gpw), c_pass = (8.0 + (double)((S + L - 1) / L)) * (L <= 2 ? 1.2 : 1.0);
    const int wpc = 4 * workgroups_per_chain(m, L, nchains, resident_workgroups(m, 0));
    const double t = ceil(npass / wpc) * c_pass;           // passes of the busiest wavefront x pass cost
    if (t < best) { best = t; bestL = L; }
  }
  const int L = m->L_override > 0 ? m->L_override : bestL;
  if (L != m->L) {
    drop_plans(m);
    m->L = L;
  }
  m->nblocks_chosen = workgroups_per_chain(m, m->L, nchains, resident_workgroups(m, 0)) * nchains;
}
// the ranges for a launch of `nch` chains beside `reserve` other workgroups
int plan_launch(ppcx_model* m, int nch, int reserve, bool trim, int* nbpc_out, const int** d_bounds_out) {
  std::lock_guard<std::mutex> lk(m->plan_mutex);
  const int n_res = resident_workgroups(m, reserve);
  const auto key = std::make_pair(nch, trim ? -n_res : n_res);   // (a trimmed plan under its own key)
  auto it = m->plans.find(key);
  if (it != m->plans.end()) { *nbpc_out = it->second.nbpc; *d_bounds_out = it->second.d_bounds.p; return PPCX_OK; }
  const int G = m->d.G, L = m->L, gpw = 64 / L;
  // beside state machines (reserve > 0) the last run of the launch may be partial: their slots and the range blocks
  // together fill the chip
  const int nbpc = workgroups_per_chain(m, L, nch, n_res, reserve == 0, trim), wpc = 4 * nbpc, npass = (G + gpw - 1) / gpw;
  std::vector<double> cost(npass);
  double total = 0;
  for (int k = 0; k < npass; ++k) {
    const int p = k * gpw;
    cost[k] = pass_cost(m, L, p, G - p < gpw ? G - p : gpw);
    total += cost[k];
  }
  // boundary j where the running cost crosses j / wpc of the total, at the nearest whole pass
  std::vector<int> bounds(wpc + 1, G);
  bounds[0] = 0;
  {
    int k = 0; double cum = 0.0;
    for (int j = 1; j < wpc; ++j) {
      const double target = total * (double)j / (double)wpc;
      while (k < npass && cum + 0.5 * cost[k] < target) cum += cost[k++];
      bounds[j] = k * gpw < G ? k * gpw : G;
    }
  }
  // no wavefront gets more than its share of passes rounded up: the four wavefronts of a SIMD take turns on its fp64
  // unit, so the launch lasts as long as the SIMD with the most passes (measured: the 8 SIMDs whose wavefronts all had
  // one pass more than the rest finished 8 us after the others, profiles/r02_wave_trace.txt)
  {
    const long pmax = ((long)(npass + wpc - 1) / wpc) * gpw;
    for (int j = 0; j < wpc; ++j) if (bounds[j + 1] - bounds[j] > pmax) bounds[j + 1] = (int)(bounds[j] + pmax);
    bounds[wpc] = G;
    for (int j = wpc - 1; j >= 0; --j) if (bounds[j + 1] - bounds[j] > pmax) bounds[j] = (int)(bounds[j + 1] - pmax);
  }
  DeviceBuffer<int> d_bounds;                    // (a failure below frees it)
  HIPCHK(d_bounds.alloc((size_t)(wpc + 1)));
  HIPCHK(hipMemcpy(d_bounds.p, bounds.data(), sizeof(int) * (size_t)(wpc + 1), hipMemcpyHostToDevice));
  ppcx_model::Plan& pl = m->plans[key];
  pl.nbpc = nbpc; std::swap(pl.d_bounds.p, d_bounds.p);
  *nbpc_out = pl.nbpc; *d_bounds_out = pl.d_bounds.p;
  return PPCX_OK;
}

static int upload_counts(ppcx_model* m, int n_excl, const int32_t* excl) {
  const int G = m->d.G, S = m->d.S, C = m->d.C;
  std::vector<int32_t> cnt(m->counts_host);
  for (int e = 0; e < n_excl; ++e) {
    if (excl[e] < 0 || excl[e] >= G * S) return fail(PPCX_ERR_ARG, "excluded cell id out of range");
    cnt[excl[e]] = -1;
  }
  std::vector<double> Sy(G, 0.0), SyE(G, 0.0), SyX((size_t)C * G, 0.0), SX((size_t)C * G, 0.0), ncell(G, 0.0), Lg1(G, 0.0);
  std::vector<unsigned char> gflags(G, 0);
  for (int g = 0; g < G; ++g) {
    double sy = 0, sye = 0, nc = 0, lg1 = 0;
    for (int s = 0; s < S; ++s) {
      const int y = cnt[(size_t)g * S + s];
      if (y < 0) { gflags[g] |= 1; continue; }
      sy += y; sye += (double)y * m->expo_host[s]; nc += 1.0; lg1 += lgamma((double)y + 1.0);
      for (int c = 0; c < C; ++c) { SyX[(size_t)c * G + g] += (double)y * m->X_host[(size_t)c * S + s]; SX[(size_t)c * G + g] += m->X_host[(size_t)c * S + s]; }
    }
    Sy[g] = sy; SyE[g] = sye; ncell[g] = nc; Lg1[g] = lg1;
  }
  HIPCHK(hipMemcpy(m->d_gflags.p, gflags.data(), (size_t)G, hipMemcpyHostToDevice));
  // gene_order: a wavefront holds several genes and runs the cell path its most demanding gene needs -- the slope columns if
  // one of them has slopes, the test for excluded cells if one of them has such cells. So neighbours in the launch should be
  // alike: genes with slopes first, among them and among the plain ones those with excluded cells first. Every count costs the
  // same since round 5 (ppcx_disp.h), so nothing else distinguishes two genes.
  {
    std::vector<int> ord(G);
    for (int g = 0; g < G; ++g) ord[g] = g;
    const int K = m->d.K;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
      const bool sa = a < K && C >= 2, sb = b < K && C >= 2;
      if (sa != sb) return sa;
      return gflags[a] > gflags[b];
    });
    // ... and the genes with slopes are dealt over the whole order in blocks of kOrderBlock positions (whole passes for every L
    // >= 4), evenly spaced among the plain genes' blocks: a wavefront's range is a contiguous piece of the order, a workgroup's
    // four wavefronts hold neighbouring ranges and a CU four workgroups in dispatch order, so with the slope genes at the front
    // a few CUs ran nothing but the dearer passes -- `~ group + age` at BASELINE size: 61 us per 8-chain launch whatever weight
    // the plan gave those passes, 46 us dealt out, against 40 us for the sum of the work; the order does not enter a gene's sums.
    // Only where those passes are much dearer (an exp per cell): with indicator columns they cost 1.15 x a plain one, and dealing
    // them out makes a chain group's launch of three chains 5 % slower (17.6 -> 18.6 us: shorter runs of alike passes).
    {
      int ns = 0;
      while (ns < G && ord[ns] < K && C >= 2) ++ns;         // genes with slopes: the first ns positions
      constexpr int kOrderBlock = 16;
      const int nbs = (ns + kOrderBlock - 1) / kOrderBlock, nb = (G + kOrderBlock - 1) / kOrderBlock;
      const bool dear_slopes = m->d.x0_is_one && !m->d.x1_binary;      // an exp per cell (sweep_cells MODE 3): 2.4 x a plain pass
      if (ns > 0 && ns < G && nbs < nb && dear_slopes) {
        std::vector<int> mixed; mixed.reserve(G);
        int is = 0, ip = ns, sb = 0;                       // next slope gene, next plain gene, slope blocks placed
        for (int b = 0; b < nb; ++b) {
          const bool slope_block = sb < nbs && b == (int)((long long)sb * nb / nbs);
          if (slope_block && is < ns) { for (int k = 0; k < kOrderBlock && is < ns; ++k) mixed.push_back(ord[is++]); ++sb; }
          else { for (int k = 0; k < kOrderBlock && ip < G; ++k) mixed.push_back(ord[ip++]); }
        }
        while (is < ns) mixed.push_back(ord[is++]);
        while (ip < G) mixed.push_back(ord[ip++]);
        ord.swap(mixed);
      }
    }
    HIPCHK(hipMemcpy(m->d_order.p, ord.data(), sizeof(int) * (size_t)G, hipMemcpyHostToDevice));
    m->pos_slope.resize(G);
    for (int p = 0; p < G; ++p) m->pos_slope[p] = ord[p] < K && C >= 2;
    drop_plans(m);
  }
  HIPCHK(hipMemcpy(m->d_counts.p, cnt.data(), sizeof(int32_t) * cnt.size(), hipMemcpyHostToDevice));
  m->excluded_host.assign(cnt.size(), 0);
  for (size_t i = 0; i < cnt.size(); ++i) m->excluded_host[i] = cnt[i] < 0;
  // the dispersion tables of all genes from the counts now on the device (a few milliseconds; excluded cells are left out of them)
  {
    const hipError_t e = launch_disp_build_kernel(m->d_counts.p, G, S, nullptr, G, m->fit, m->d_disp.p, m->stream.s);
    if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("dispersion-table kernel: ") + hipGetErrorString(e));
  }
  HIPCHK(hipMemcpy(m->d_Sy.p, Sy.data(), sizeof(double) * G, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_SyE.p, SyE.data(), sizeof(double) * G, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_SyX.p, SyX.data(), sizeof(double) * SyX.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_SX.p, SX.data(), sizeof(double) * SX.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_ncell.p, ncell.data(), sizeof(double) * G, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_Lg1.p, Lg1.data(), sizeof(double) * G, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(m->stream.s));
  return PPCX_OK;
}

// per_sample: where the log-likelihood kernel keeps the per-sample constants (ppcx.h PPCX_PER_SAMPLE_*)
static int model_create(int device, int G, int S, int C, int K, const int32_t* counts, const double* X, const double* exposure,
                        double lambda_mu_mu, int n_excl, const int32_t* excl, int per_sample, ppcx_model** out) {
  if (!out) return fail(PPCX_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (per_sample != PPCX_PER_SAMPLE_LDS && per_sample != PPCX_PER_SAMPLE_STREAM && per_sample != PPCX_PER_SAMPLE_AUTO)
    return fail(PPCX_ERR_ARG, "per_sample must be PPCX_PER_SAMPLE_LDS, PPCX_PER_SAMPLE_STREAM or PPCX_PER_SAMPLE_AUTO");
  if (G < 1 || S < 1 || C < 1 || K < 0 || K > G) return fail(PPCX_ERR_ARG, "need G>=1, S>=1, C>=1, 0<=K<=G");
  if (C > kMaxC) return fail(PPCX_ERR_LIMIT, "C exceeds the 16 design columns this build supports");
  if ((long long)G * S > 2000000000LL) return fail(PPCX_ERR_LIMIT, "G*S exceeds int32 cell ids");
  if (!counts || !X || !exposure || (n_excl > 0 && !excl)) return fail(PPCX_ERR_ARG, "NULL input buffer");
  for (long long i = 0; i < (long long)G * S; ++i) if (counts[i] < 0) return fail(PPCX_ERR_ARG, "negative count");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PPCX_ERR_ARG, "no such HIP device");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<ppcx_model> owner(new ppcx_model());   // every return before the last frees the model (its device is current)
  ppcx_model* m = owner.get();
  m->device = device;
  m->d = make_dims(G, S, C, K, lambda_mu_mu);
  m->CM = C <= 2 ? 2 : (C <= 4 ? 4 : (C <= 8 ? 8 : 16));
  {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    m->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  m->counts_host.assign(counts, counts + (size_t)G * S);
  m->X_host.assign(X, X + (size_t)S * C);
  m->expo_host.assign(exposure, exposure + S);
  int x0 = 1;
  for (int s = 0; s < S; ++s) if (X[s] != 1.0) x0 = 0;
  m->d.x0_is_one = x0;
  int x1b = (C >= 2);                          // factor design: every slope column is a 0 / 1 indicator (C == 2: two groups)
  for (size_t i = (size_t)S; i < (size_t)S * C && x1b; ++i) if (X[i] != 0.0 && X[i] != 1.0) x1b = 0;
#ifdef PPCX_TESTING
  if (g_test.force_generic) x1b = 0;
#endif
  m->d.x1_binary = x1b;
  m->d.raw_consts = (!x0 || (C >= 2 && K > 0 && !x1b)) ? 1 : 0;
  // more than 8 design columns: the instantiation for factor designs only (a twelve-level factor, `~ a + b + c` of factors:
  // model.matrix columns that are all indicators, R/utilities.R:887-900); a continuous covariate among more than 8 columns,
  // or such a design without the column of ones, has no instantiation in this build
  if (C > 8 && (!x0 || (K > 0 && !x1b)))
    return fail(PPCX_ERR_LIMIT, "more than 8 design columns are supported for designs of a column of ones and 0 / 1 indicator columns only");
  // the two tuning knobs of a fit's round structure, read from the environment HERE and nowhere else
  if (const char* e = getenv("PPCX_PIPELINE")) if (atoi(e) == 0) m->opt_pipelined = 0;
  if (const char* e = getenv("PPCX_STREAM_GROUPS")) { const int v = atoi(e); if (v >= 1) m->opt_stream_groups = v; }
  // the log-likelihood kernel stages its tables (20 KB) and the per-sample constants in LDS: exp(exposure) and the design's slope
  // columns -- S * C doubles; S * (2 + C) without the column of ones. Beyond that a model streams them from global memory if it was
  // asked to (ppcx_model_create_ex): the same sweep on the model's own arrays, in the three-launch round only -- the merged launch
  // of a pipelined round has no streamed form, so such a model reports no resident workgroups for it (model_pipelines)
  const bool fits_lds = loglik_lds_bytes(m->d, false) <= 160u * 1024u;
  m->streamed = per_sample == PPCX_PER_SAMPLE_STREAM || (per_sample == PPCX_PER_SAMPLE_AUTO && !fits_lds);
  if (!m->streamed && !fits_lds)
    return fail(PPCX_ERR_LIMIT, "the per-sample constants (S * C doubles; S * (2 + C) for a design without a column of ones) do not fit the 160 KB of LDS of a compute unit beside the 20 KB of tables");
  // ... and then the next bound is the dispersion-table kernel's, which keeps a gene's row of S counts in LDS
  if (m->streamed && disp_build_lds_bytes(S) > 160u * 1024u)
    return fail(PPCX_ERR_LIMIT, "the dispersion-table kernel (ppcx_disp_build_kernel) keeps a gene's row of S counts in LDS beside 5.5 KB of node values: S may not exceed 39 552");
  m->wgs_per_cu = loglik_resident_workgroups_per_cu(m->CM, m->d, m->streamed);      // of the instantiation this model runs
  if (m->wgs_per_cu < 1) return fail(PPCX_ERR_LIMIT, "the log-likelihood kernel cannot be resident with S * (2 + C) doubles of per-sample constants in LDS");
  m->ls_wgs_per_cu = m->streamed ? 0 : ls_resident_workgroups_per_cu(m->CM, m->d);
  std::vector<double> E(S);
  for (int s = 0; s < S; ++s) E[s] = exp(exposure[s]);
  HIPCHK(m->stream.create());
  HIPCHK(m->d_counts.alloc(((size_t)G * S + 512)));   // + 512: the row sweep requests counts up to two trips of 4 x 64 lanes past the end
  HIPCHK(hipMemset(m->d_counts.p, 0, sizeof(int32_t) * ((size_t)G * S + 512)));
  // a streamed model's sweep reads exp(exposure) and the last column of X up to kLdsPad entries past their ends (sweep_cells: the
  // partial last trip, the trip requested ahead), as the LDS route reads its copies: padded with finite values that no cell uses
  const size_t pad = m->streamed ? (size_t)kLdsPad : 0;
  HIPCHK(m->d_E.alloc(S + pad));
  HIPCHK(m->d_expo.alloc(S + pad));
  HIPCHK(m->d_X.alloc((size_t)S * C + pad));
  HIPCHK(m->d_Sy.alloc(G));
  HIPCHK(m->d_SyE.alloc(G));
  HIPCHK(m->d_SyX.alloc((size_t)C * G));
  HIPCHK(m->d_SX.alloc((size_t)C * G));
  HIPCHK(m->d_ncell.alloc(G));
  HIPCHK(m->d_disp.alloc((size_t)G * kDispGeneDoubles));
  HIPCHK(m->d_gflags.alloc((size_t)G));
  disp_fit_init(m->fit);
  HIPCHK(m->d_Lg1.alloc(G));
  HIPCHK(m->d_logtab.alloc(2 * kLogTabSize));
  { double tab[2 * kLogTabSize]; fill_log_table(tab); HIPCHK(hipMemcpy(m->d_logtab.p, tab, sizeof(tab), hipMemcpyHostToDevice)); }
  HIPCHK(m->d_wintab.alloc(2 * kWinTabSize));
  { std::vector<double> wt(2 * kWinTabSize); fill_window_log_table(wt.data()); HIPCHK(hipMemcpy(m->d_wintab.p, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice)); }
  m->e_min = m->e_max = E[0];
  for (int s = 1; s < S; ++s) { if (E[s] < m->e_min) m->e_min = E[s]; if (E[s] > m->e_max) m->e_max = E[s]; }
  HIPCHK(m->d_order.alloc((size_t)G));
  HIPCHK(hipMemcpy(m->d_E.p, E.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_expo.p, exposure, sizeof(double) * S, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_X.p, X, sizeof(double) * (size_t)S * C, hipMemcpyHostToDevice));
  if (pad) {
    HIPCHK(hipMemset(m->d_E.p + S, 0, sizeof(double) * pad));
    HIPCHK(hipMemset(m->d_expo.p + S, 0, sizeof(double) * pad));
    HIPCHK(hipMemset(m->d_X.p + (size_t)S * C, 0, sizeof(double) * pad));
  }
  const int rc = upload_counts(m, n_excl, excl);
  if (rc != PPCX_OK) return rc;
  choose_launch(m, 1);
  *out = owner.release();
  return PPCX_OK;
}
extern "C" int ppcx_model_create(int device, int G, int S, int C, int K, const int32_t* counts, const double* X,
                                 const double* exposure, double lambda_mu_mu, int n_excl, const int32_t* excl,
                                 ppcx_model** out) {
  return model_create(device, G, S, C, K, counts, X, exposure, lambda_mu_mu, n_excl, excl, PPCX_PER_SAMPLE_LDS, out);
}
extern "C" int ppcx_model_create_ex(int device, int G, int S, int C, int K, const int32_t* counts, const double* X,
                                    const double* exposure, double lambda_mu_mu, int n_excl, const int32_t* excl,
                                    int per_sample, ppcx_model** out) {
  return model_create(device, G, S, C, K, counts, X, exposure, lambda_mu_mu, n_excl, excl, per_sample, out);
}
extern "C" int ppcx_model_get_per_sample(const ppcx_model* m, int* streamed) {
  if (!m || !streamed) return fail(PPCX_ERR_ARG, "bad arguments");
  *streamed = m->streamed ? 1 : 0;
  return PPCX_OK;
}
// ---- gene shards (second mode; the reference's map_rect over gene shards, .stan:226-240) ---------
extern "C" int ppcx_model_create_shard_strided(int device, int G_total, int S, int C, int K_total, int g0, int gene_stride, int n_genes,
                                               const int32_t* counts_shard, const double* X, const double* exposure,
                                               double lambda_mu_mu, int n_excl, const int32_t* excl_local, ppcx_model** out) {
  if (g0 < 0 || gene_stride < 1 || n_genes < 1 || K_total < 0 || K_total > G_total ||
      (long long)g0 + (long long)gene_stride * (n_genes - 1) >= G_total) return fail(PPCX_ERR_ARG, "bad gene shard");
  // the shard's checked genes: its genes among the first K_total of the whole problem (they come first in the shard too)
  int kl = 0;
  if (g0 < K_total) kl = (K_total - g0 + gene_stride - 1) / gene_stride;
  if (kl > n_genes) kl = n_genes;
  int rc = ppcx_model_create(device, n_genes, S, C, kl, counts_shard, X, exposure, lambda_mu_mu, n_excl, excl_local, out);
  if (rc != PPCX_OK) return rc;
  (*out)->d.Gt = G_total; (*out)->d.Kt = K_total; (*out)->d.g0 = g0; (*out)->d.k0 = g0 < K_total ? g0 : K_total; (*out)->d.gstride = gene_stride;
  return PPCX_OK;
}
extern "C" int ppcx_model_create_shard(int device, int G_total, int S, int C, int K_total, int g0, int g1,
                                       const int32_t* counts_shard, const double* X, const double* exposure,
                                       double lambda_mu_mu, int n_excl, const int32_t* excl_local, ppcx_model** out) {
  if (g0 < 0 || g1 <= g0 || g1 > G_total) return fail(PPCX_ERR_ARG, "bad gene range");
  return ppcx_model_create_shard_strided(device, G_total, S, C, K_total, g0, 1, g1 - g0, counts_shard, X, exposure, lambda_mu_mu, n_excl, excl_local, out);
}

extern "C" int ppcx_model_set_exclusions(ppcx_model* m, int n_excl, const int32_t* excl) {
  if (!m || (n_excl > 0 && !excl) || n_excl < 0) return fail(PPCX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(m->device));
  return upload_counts(m, n_excl, excl);
}
extern "C" int ppcx_model_set_launch(ppcx_model* m, int lanes_per_gene, int workgroups) {
  if (!m) return fail(PPCX_ERR_ARG, "model is NULL");
  if (lanes_per_gene != 0 && (lanes_per_gene < 1 || lanes_per_gene > 64 || (lanes_per_gene & (lanes_per_gene - 1))))
    return fail(PPCX_ERR_ARG, "lanes_per_gene must be 0 or a power of two <= 64");
  if (workgroups < 0 || workgroups > (1 << 20)) return fail(PPCX_ERR_ARG, "workgroups must be 0 (automatic) or a positive count");
  HIPCHK(hipSetDevice(m->device));
  m->L_override = lanes_per_gene; m->wgs_override = workgroups;
  drop_plans(m);
  choose_launch(m, 1);
  return PPCX_OK;
}
extern "C" int ppcx_model_set_rounds(ppcx_model* m, int pipelined, int stream_groups) {
  if (!m) return fail(PPCX_ERR_ARG, "model is NULL");
  if (pipelined < -2 || pipelined > 1 || stream_groups < -1 || stream_groups > 64) return fail(PPCX_ERR_ARG, "pipelined must be -2 .. 1 and stream_groups -1 .. 64");
  if (pipelined != -2) m->opt_pipelined = pipelined;           // -2 / -1: leave that setting as it is
  if (stream_groups != -1) m->opt_stream_groups = stream_groups;
  return PPCX_OK;
}
bool model_pipelines(const ppcx_model* m) {
  // the pipelined round needs cells that read the anticipated constants only: every design since round 5 (a per-cell linear
  // predictor reads the coefficients kept among the constants: Dims::raw_consts); a streamed model has no merged launch
  return m->opt_pipelined != 0 && m->ls_wgs_per_cu >= 1;
}
extern "C" int ppcx_model_set_progress(ppcx_model* m, ppcx_progress_fn fn, void* user, double every_seconds) {
  if (!m || !(every_seconds >= 0)) return fail(PPCX_ERR_ARG, "bad arguments");
  m->progress = fn; m->progress_user = user; m->progress_every = every_seconds;
  return PPCX_OK;
}
extern "C" int ppcx_model_get_rounds(const ppcx_model* m, int nchains, int* pipelined, int* stream_groups) {
  if (!m || nchains < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  if (pipelined) *pipelined = model_pipelines(m) ? 1 : 0;
  if (stream_groups) *stream_groups = fit_stream_groups(m, nchains);
  return PPCX_OK;
}
extern "C" int ppcx_model_get_launch(const ppcx_model* m, int* lanes_per_gene, int* nblocks) {
  if (!m) return fail(PPCX_ERR_ARG, "model is NULL");
  if (lanes_per_gene) *lanes_per_gene = m->L;
  if (nblocks) *nblocks = m->nblocks_chosen;
  return PPCX_OK;
}
// the plan of a log-likelihood launch of `nchains` chains: workgroups per chain, and the gene-order positions
// bounds[0 .. 4 * workgroups_per_chain] that delimit the wavefronts' ranges (bounds may be NULL; `cap` entries at most).
// A diagnostic: tests check its invariants, nothing in the product path reads it back.
extern "C" int ppcx_model_get_plan(ppcx_model* m, int nchains, int* lanes_per_gene, int* workgroups_per_chain, int* bounds, int cap) {
  if (!m || nchains == 0) return fail(PPCX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(m->device));
  // nchains < 0: the launch of -nchains chains of ONE of several chain groups (trimmed: workgroups_per_chain), at the lanes
  // per gene in force -- those of the fit, chosen for all its chains
  const bool trim = nchains < 0;
  if (trim) nchains = -nchains; else choose_launch(m, nchains);
  int nbpc = 0; const int* d_bounds = nullptr;
  const int rc = plan_launch(m, nchains, 0, trim, &nbpc, &d_bounds);
  if (rc != PPCX_OK) return rc;
  if (lanes_per_gene) *lanes_per_gene = m->L;
  if (workgroups_per_chain) *workgroups_per_chain = nbpc;
  if (bounds) {
    const int n = 4 * nbpc + 1;
    if (cap < n) return fail(PPCX_ERR_ARG, "bounds buffer too small");
    HIPCHK(hipMemcpy(bounds, d_bounds, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  }
  return PPCX_OK;
}
extern "C" int ppcx_model_dim(const ppcx_model* m) { return m ? m->d.D : PPCX_ERR_ARG; }
extern "C" void ppcx_model_destroy(ppcx_model* m) {
  if (!m) return;
  if (m->live_fits > 0) { m->destroy_requested = true; return; }   // freed by the last ppcx_fit_free
  (void)hipSetDevice(m->device);               // the model's stream and buffers go on its device
  delete m;
}

#ifdef PPCX_TESTING
// ---- testing build only (ppcx_testing.h) ---------------------------------------------------------------------------
extern "C" int ppcx_testing_set(const char* key, long long value) {
  if (!key) return fail(PPCX_ERR_ARG, "key is NULL");
  const std::string k(key);
  if (k == "fail_at_round") g_test.fail_at_round = value;
  else if (k == "fail_rank") g_test.fail_rank = (int)value;
  else if (k == "force_generic") g_test.force_generic = (int)value;
  else if (k == "slope_cost_permille") g_test.slope_cost_permille = (int)value;
  else if (k == "trim_slack_permille") g_test.trim_slack_permille = (int)value;
  else if (k == "trim_extra_passes") g_test.trim_extra_passes = (int)value;
  else if (k == "psis_slots") g_test.psis_slots = (int)value;
  else if (k == "psis_scratch_bytes") g_test.psis_scratch_bytes = value;
  else if (k == "loo_scratch_bytes") g_test.loo_scratch_bytes = value;
  else return fail(PPCX_ERR_ARG, "unknown test hook " + k);
  return PPCX_OK;
}
extern "C" int ppcx_testing_get_disp_table(ppcx_model* m, double* out) {
  if (!m || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream.s));
  HIPCHK(hipMemcpy(out, m->d_disp.p, sizeof(double) * (size_t)m->d.G * kDispGeneDoubles, hipMemcpyDeviceToHost));
  return PPCX_OK;
}
#endif
