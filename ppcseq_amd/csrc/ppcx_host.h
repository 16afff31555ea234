// ppcx_host.h -- what the host translation units of the C ABI share (ppcx_capi.hip, ppcx_run.hip, ppcx_fit_nuts.hip,
// ppcx_fit_advi.hip, ppcx_fit_api.hip; no kernel includes it): the error state, the testing build's hooks, what a model, a fit
// and a run hold, and the functions that cross those files. Everything here has hidden visibility (the build's default).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/ppcx.h"
#include "ppcx_kernels.h"
#include "ppcx_columns.h"

using namespace ppcx;

// the last error of the calling thread (ppcx_last_error): one object for the whole library, defined in ppcx_capi.hip
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
// a HIP error as a status: `what` is the failed expression (HIPCHK) or the name of the step
int hip_fail(hipError_t e, const char* what);
// the end of an entry point: the driver's error as PPCX_ERR_HIP under the entry's name (null: the bare text)
int hip_done(const char* who, hipError_t e);
#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);                                      \
  } while (0)

// Test hooks exist only in the testing build (-DPPCX_TESTING: tests/libppcx_testing.so, built by __graft_entry__.build()
// for tests/ and scripts/); the shipped library has none of them and reads no environment variable after model creation.
#ifdef PPCX_TESTING
#include "ppcx_testing.h"
struct TestHooks {
  long long fail_at_round = 0; int fail_rank = -1;   // fault injection into the pump of a gene-sharded run
  int force_generic = 0;                             // every gene with slopes takes the per-cell-eta path
  int slope_cost_permille = 0;                       // plan: cost of a pass with slope genes relative to a plain one (0: built-in)
  int trim_slack_permille = -1;                      // plan: slack of a chain group's trimmed launch (-1: built-in)
  int trim_extra_passes = 0;                         // plan: passes per wavefront of a trimmed launch beyond the fewest possible
  int psis_slots = 0;                                // Pareto-k diagnostic: draws evaluated per launch for log_p (0: built-in)
  long long psis_scratch_bytes = 0;                  // ... bound of its column scratch per batch (0: built-in)
  long long loo_scratch_bytes = 0;                   // PSIS-LOO: bound of the gene table / column scratch per batch (0: built-in)
  std::string rccl_lib;                              // another provider of the nccl* entry points (tests/loopback)
};
extern TestHooks g_test;                            // (ppcx_capi.hip)
#endif

// The model owns its stream and its device memory: they go with it (ppcx_model_destroy, on the model's device).
struct ppcx_model {
  int device;
  DeviceStream stream;                         // declared before every buffer: destroyed after them
  Dims d;
  int CM, L = 64;
  int L_override = 0, wgs_override = 0;        // ppcx_model_set_launch
  int n_cu = 256, wgs_per_cu = 4;              // resident workgroups of the log-likelihood kernel = n_cu * wgs_per_cu
  int ls_wgs_per_cu = 0;                       // the same for the merged launch of a pipelined round (0: cannot run)
  bool streamed = false;                       // the log-likelihood kernel reads the per-sample constants from global memory, not from
                                               // LDS (ppcx_model_create_ex): d_E, d_expo, d_X carry kLdsPad entries more
  int nblocks_chosen = 0;                      // workgroups of the last planned launch (what ppcx_model_get_launch reports)
  // round structure of a NUTS fit (ppcx_model_set_rounds; initial values from PPCX_PIPELINE / PPCX_STREAM_GROUPS, read
  // once when the model is created): pipelined -1 = where it applies, 0 = never; stream_groups 0 = by the number of chains
  int opt_pipelined = -1, opt_stream_groups = 0;
  // progress reports of a running fit (ppcx_model_set_progress): the pump calls it at a poll, at most every progress_every s
  ppcx_progress_fn progress = nullptr; void* progress_user = nullptr; double progress_every = 1.0;
  // gene order of the log-likelihood launch (upload_counts): per position, whether the gene has slopes -- what a pass of a
  // wavefront costs (plan_launch)
  std::vector<char> pos_slope;
  struct Plan { int nbpc = 0; DeviceBuffer<int> d_bounds; };
  std::map<std::pair<int, int>, Plan> plans;   // (chains in the launch, resident workgroups it may use) -> ranges
  std::mutex plan_mutex;
  std::vector<int32_t> counts_host;            // original counts (exclusions are re-applied on a copy)
  std::vector<char> excluded_host;             // [G][S] the cells excluded now (ppcx_fit_loo holds them out)
  std::vector<double> X_host, expo_host;
  DeviceBuffer<int> d_counts;
  DeviceBuffer<double> d_E, d_expo, d_X, d_Sy, d_SyE, d_SyX, d_SX, d_ncell, d_Lg1;
  DeviceBuffer<double> d_disp;                 // [G][kDispGeneDoubles] the genes' dispersion tables (ppcx_disp.h)
  DeviceBuffer<unsigned char> d_gflags;        // [G] bit 0: the gene has excluded cells
  DispFit fit;                                 // nodes and transforms of the table build
  DeviceBuffer<double> d_logtab, d_wintab;
  double e_min = 1.0, e_max = 1.0;             // smallest and largest exp(exposure_s)
  DeviceBuffer<int> d_order;     // gene_order: position in the log-likelihood kernel's launch -> gene
  int live_fits = 0;             // fits that still point at this model: ppcx_model_destroy defers until the last one is freed
  bool destroy_requested = false;
};

struct ppcx_fit {
  ppcx_model* m;
  NutsConfig cfg;
  int chains, n_keep, iter;
  // the fit owns its device buffers: they go with it (ppcx_fit_free, on the model's device); .p stays null where a fit has none
  DeviceBuffer<double> d_draws;                // [chains][n_keep][D] (none without kept draws)
  DeviceBuffer<double> d_lp, d_stepsize, d_accept;   // lp [chains][n_keep] (none without kept draws, none over draws made elsewhere)
  DeviceBuffer<int> d_treedepth, d_nleap, d_div;     // the diagnostics [chains][iter] each
  double seconds = 0; long long grad_evals = 0;
  double kA_ms_mean = 0; long long kA_samples = 0; double kA_chain_launches_mean = 0;
  double kC_ms_mean = 0, kU_ms_mean = 0; long long launch_triples = 0;
  double advi_elbo = 0, advi_eta = 0; int advi_converged = 0;
  double ppc_ms = 0; long long ppc_draws = 0;  // last ppcx_fit_ppc: kernel time (HIP events) and NB draws generated
  long long xchg_ticks = 0, xchg_count = 0;    // direct exchange: 100 MHz ticks the chains' state machines waited for peers, exchanges
  std::vector<double> inv_metric;              // [chains][D] diagonal of the adapted inverse metric (host; ppcx_fit_get_inv_metric)
  bool advi = false;                           // draws of an ADVI approximation (independent: ppcx_fit_summary refuses them)
  DeviceBuffer<double> d_mu, d_omega;          // ADVI: the fitted approximation [D] each (ppcx_fit_get_approximation)
  DeviceBuffer<double> d_log_p, d_log_g, d_r;  // ADVI: log densities and log ratios at the kept draws
                                               // [n_keep] each, made by the first ppcx_fit_get_log_ratios / ppcx_fit_psis
};
inline void fit_attach(ppcx_fit* f, ppcx_model* m) { f->m = m; m->live_fits++; }

// device scratch of one run of the launch pump. States, commands, hyper-coordinate vectors and the T0 slab
// are double-buffered: update launch k reads buffer k&1 and writes buffer (k+1)&1.
struct Work {
  DeviceStream own;              // a chain group's stream, where the run has one of its own (declared first: destroyed last)
  hipStream_t stream = nullptr;  // the stream of the run: own.s, or borrowed from the model (work_alloc)
  DeviceBuffer<double> vecs, hyper_vecs[2], partials, t0[2], sums, red;
  DeviceBuffer<Cmd> cmds[2]; DeviceBuffer<ChainState> states[2]; DeviceBuffer<int> done;
  PinnedBuffer<int> done_host;
  long Dpad = 0; int nb_update = 1, nb_close = 1; long launches = 0;
  bool pipelined = false;        // two launches per round (ppcx_ls_kernel + ppcx_gene_kernel) instead of three
  bool shared_chip = false;      // one of several chain groups of a fit: its launches leave the slots they cannot use (workgroups_per_chain)
  std::atomic<int>* stop = nullptr;   // shared by the chain groups of a fit: set when the progress callback ended one of them
  DeviceBuffer<int> active; PinnedBuffer<int> active_host; int n_active = 0;   // chains still running (pump), 0 = all
  const XchgArgs* xchg = nullptr; int xchg_chain0 = 0;   // gene shards with the direct exchange: the group's first chain in the buffers
};
struct RunIO {                  // output buffers of a run (device pointers, may be null)
  double* draws = nullptr; long draws_stride = 0; int n_keep = 0, iter = 0;
  double *lp = nullptr, *stepsize = nullptr, *accept = nullptr; int *treedepth = nullptr, *nleap = nullptr, *div = nullptr;
};
inline ChainState* current_states(Work& w) { return w.states[w.launches & 1].p; }
inline double* current_hyper(Work& w) { return w.hyper_vecs[w.launches & 1].p; }

struct PumpStats { double kA_ms_sum = 0, kC_ms_sum = 0, kU_ms_sum = 0; long long kA_samples = 0; double chain_launches = 0; long long pairs = 0; };
// One shard of a run: its model (all genes, or a contiguous gene range) and its device scratch.
struct Shard { ppcx_model* m; Work* w; RunIO io; };

// ---- ppcx_capi.hip: the launch geometry
void choose_launch(ppcx_model* m, int nchains);
int fit_stream_groups(const ppcx_model* m, int nch);   // chain groups of a fit of `nch` chains
int fit_launch_chains(const ppcx_model* m, int nch);   // chains in a launch of such a fit
int plan_launch(ppcx_model* m, int nch, int reserve, bool trim, int* nbpc, const int** d_bounds);
bool model_pipelines(const ppcx_model* m);

// ---- ppcx_run.hip: a run's scratch, its launches and the pump
int work_alloc(Work& w, ppcx_model* m, int nchains);
int launch_step(ppcx_model* m, Work& w, int nchains, const RunIO& io, int phases, bool with_update = false);
int launch_update(ppcx_model* m, Work& w, int nchains, const RunIO& io);
int launch_loglik(ppcx_model* m, Work& w, int nchains);
int launch_close(ppcx_model* m, Work& w, int nchains);
int pump(std::vector<Shard>& sh, int nchains, ppcx_comm* comm, long long max_pairs, bool time_kernels, PumpStats* stats);
int pump(ppcx_model* m, Work& w, int nchains, const RunIO& io, long long max_pairs, bool time_kernels, PumpStats* stats,
         ppcx_comm* comm = nullptr);

// ---- ppcx_fit_advi.hip: log_p - log_g at the kept draws of an ADVI fit, cached on the fit
int psis_ratios(ppcx_fit* f);
