// ppcx_kernels.h -- argument blocks, launchers and drivers of the gfx950 kernels (the ppcx_kernels*.hip translation units of the
// NB hierarchical NUTS / ADVI engine, one per kernel family, and the translation units of the predictive kernels and the fit
// diagnostics).
//
// The engine's kernels and the translation unit that holds each, with its launch helpers:
//   ppcx_loglik_kernel<CM,GEN>  ppcx_kernels.hip        streams the int32 count matrix once per gradient evaluation and reduces it
//                           to a handful of sums per gene. Replaces lp_reduce + map_rect + X*alpha of
//                           inst/stan/negBinomial_MPI.stan:58-120,:205,:226-240. CM = design columns (2, 4, 8, 16), GEN = the
//                           route with an exp per cell that is compiled in (0 none, 1 continuous covariate, 2 no column of ones).
//   ppcx_loglik_stream_kernel<CM,GEN>  ppcx_kernels_stream.hip   the same workgroup with the per-sample constants read from global memory.
//   ppcx_ls_kernel<CM,GEN>  ppcx_kernels_ls.hip     the merged launch of a pipelined round: those workgroups beside the chains' state machines.
//   ppcx_gene_kernel<CM>    ppcx_kernels_close.hip  the other launch of a pipelined round: everything per gene (command, close, anticipated constants).
//   ppcx_close_kernel<CM>   ppcx_kernels_close.hip  per gene: priors (.stan:219-223), gradient, second half kick of the leapfrog, NUTS tree
//                           bookkeeping of the gene's coordinates, block partial sums.
//   ppcx_step_kernel        ppcx_kernels_ls.hip     reduction of the close kernel's block partials, hyper-parameters, NUTS / adaptation state
//                           machine (ppcx_nuts.h) and, in the same launch, the per-coordinate work of the next command.
//   ppcx_update_kernel      ppcx_kernels_ls.hip     that per-coordinate work as a launch of its own (initialisation, ADVI).
//   ppcx_sum_shards_kernel  ppcx_kernels_ls.hip     in-process gene shards: the sum of the shards' sums.
//   ppcx_xchg_abort_kernel  ppcx_kernels_ls.hip     a rank that leaves a gene-sharded fit says so to its peers.
//   ppcx_advi_kernel        ppcx_kernels_ls.hip     the per-coordinate work of ADVI (draws, steps); ppcx_advi_elbo_kernel its ELBO.
//   ppcx_disp_build_kernel  ppcx_kernels_model.hip  the genes' dispersion tables (ppcx_disp.h), once per model and per change of the exclusions.
//   ppcx_gather_kernel      ppcx_kernels_model.hip  column gather of the retained draws.
//   ppcx_fill_kernel        ppcx_kernels_model.hip  a constant into an array.
// The log-likelihood workgroup itself is ppcx_loglik.h, the chain's state machine ppcx_step.h (device headers). The kernels of
// ppcx_kernels_ls.hip stay together because their code depends on it (its header says how).
//
// Work decomposition of the log-likelihood kernel: a gene is owned by L lanes of one wavefront
// (L in {1,2,4,...,64}); a wavefront walks a range of the host's gene order, 64 / L genes per pass; lanes stride over the
// gene's samples four cells per trip, read the per-sample constants from LDS, and combine with an L-lane butterfly.
// Per-block partial sums of the close kernel go to a slab that the step kernel reduces in a fixed order, so results are
// bitwise reproducible for a fixed number of lanes per gene.
#pragma once
#include <hip/hip_runtime.h>
#include "ppcx_gene.h"

namespace ppcx {

// ChainState / Cmd travel between global memory, registers and LDS word by word (one 4-byte word per thread). The word type
// may alias any object: reading a struct with double members through a plain `int` lvalue is undefined under the strict
// aliasing rule that -O3 applies, whatever the copy looks like in practice.
typedef int __attribute__((may_alias)) word_t;
// v of lane i moved by a DPP control word (data-parallel primitives: a VALU move, no LDS round trip); lanes the
// control leaves without a source, or outside row_mask, receive 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_take(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
  return __hiloint2double(hi, lo);
}

constexpr int kLdsPad = 256;     // entries the sweep may read past the per-sample arrays (4 x 64 lanes), in LDS or in global memory
struct LoglikArgs {
  Dims d;
  CellData cd;                  // counts, dispersion tables, gene flags (ppcx_gene.h)
  const double* sampleE;        // exp(exposure_s)
  const double* exposure;       // S
  const double* X;              // S x C column-major
  double* vecs;                 // [chains][V_COUNT][Dpad] (read only here)
  long Dpad;
  const Cmd* cmds;              // [chains]
  double* sums;                 // [chains][3+CM][G] (GeneSumsV)
  const double* logtab;         // 2 x 256 doubles (device), ppcx_math.h table_log
  const double* wintab;         // 2 x 1024 doubles (device), ppcx_math.h window table
  const int* order;             // [G] launch position -> gene (host: gene_order)
  int lgL;                      // log2 of the lanes per gene
  int nchains;                  // chains of this launch
  const int* active;            // [nchains] their indices in cmds / vecs / sums (null: 0 .. nchains - 1)
  int nbpc;                     // workgroups per chain; wavefront j = 0 .. 4 nbpc - 1 of a chain takes the gene positions
  const int* bounds;            // [4 nbpc + 1]  bounds[j] .. bounds[j + 1] - 1 (host: plan_launch, balanced by cost)
#ifdef PPCX_TRACE               // development builds only (scripts/gpu_pass_trace.py): clock stamps of the passes' phases
  unsigned long long* trace;    // [kTraceBlocks][4 waves][kTracePasses][kTraceStamps] or null
#endif
};
#ifdef PPCX_TRACE
constexpr int kTraceBlocks = 64, kTracePasses = 8, kTraceStamps = 8;
#endif

struct CloseArgs {
  Dims d;
  const double* Sy;             // per-gene sufficient statistics over non-excluded cells
  const double* SyE;
  const double* SyX;            // [C][G]
  const double* SX;             // [C][G] sum of X_sc over the gene's non-excluded cells
  const double* ncell;          // [G] number of non-excluded cells
  const double* Lg1;            // per-gene sum of lgamma(y+1)
  const double* sums;
  double* vecs; long Dpad;
  const Cmd* cmds;
  double* partials;             // [chains][nblocks_close][PT_COUNT]
};

// the gene kernel of a pipelined round (ppcx_gene_kernel): close kernel + the per-coordinate work of the command + the
// constants of the anticipated next position
struct GeneArgs {
  CloseArgs c;
  double* draws; long draws_chain_stride;   // PRE_STORE_DRAW
  int spec;                     // anticipate the next leaf's position (models whose cell paths read the constants only)
};

// Direct exchange of a gene-sharded run (one shard per rank; the reference's map_rect over gene shards,
// inst/stan/negBinomial_MPI.stan:226-240): every rank's state machine adds the ranks' partial sums itself. Rank k's receive
// buffer is mapped into every rank (peer-mapped device memory: hipIpc handles between processes, plain pointers inside one);
// a state machine stores its PT_COUNT sums into every rank's buffer, then a sequence number, and waits until the sequence
// numbers of all ranks have arrived in its own buffer. No collective library call, no kernel boundary: the exchange happens
// inside the merged launch of a pipelined round, beside the log-likelihood workgroups.
constexpr int kMaxRanks = 16;
struct XchgArgs {
  int nranks = 1, rank = 0, max_chains = 0;
  int chain0 = 0;                              // first chain of the launch's chain group in the buffers
  unsigned epoch = 0;                          // of this fit: stale sequence numbers of earlier fits never match
  long long timeout_ticks = 0;                 // of the 100 MHz wall clock: a peer that does not arrive fails the chain
  double* recv[kMaxRanks];                     // [2 slots][nranks][max_chains][PT_COUNT]
  unsigned long long* flags[kMaxRanks];        // [2 slots][nranks][max_chains] sequence numbers, then [nranks] abort epochs
};
PPCX_HD long xchg_recv_index(const XchgArgs& x, int slot, int src, int chain) { return (((long)slot * x.nranks + src) * x.max_chains + x.chain0 + chain) * PT_COUNT; }
PPCX_HD long xchg_flag_index(const XchgArgs& x, int slot, int src, int chain) { return ((long)slot * x.nranks + src) * x.max_chains + x.chain0 + chain; }
PPCX_HD long xchg_abort_index(const XchgArgs& x, int src) { return 2L * x.nranks * x.max_chains + src; }
PPCX_HD size_t xchg_recv_doubles(int nranks, int max_chains) { return (size_t)2 * nranks * max_chains * PT_COUNT; }
PPCX_HD size_t xchg_flag_words(int nranks, int max_chains) { return (size_t)2 * nranks * max_chains + nranks; }

enum StepPhase : int { STEP_REDUCE = 1, STEP_ADVANCE = 2 };
struct StepArgs {
  Dims d;
  int phases;                   // STEP_REDUCE | STEP_ADVANCE (one launch), or the two halves around a shard exchange
  const ChainState* states_in; ChainState* states_out;   // double-buffered between rounds
  const Cmd* cmds_in; Cmd* cmds_out;
  const double* hyper_in; double* hyper_out;             // [chains][V_COUNT][8]
  const double* partials; int nblocks_close;             // [chains][slab_stride][PT_COUNT], rows 0 .. nblocks_close - 1 are summed
  int slab_stride;
  const double* t0; int nblocks_update;                  // [chains][nblocks_update]
  double* red;                                           // [chains][PT_COUNT]
  double* draws; long draws_chain_stride;
  int n_keep, iter;
  double* out_lp; double* out_stepsize; int* out_treedepth; int* out_n_leapfrog; int* out_divergent; double* out_accept;
  int* done;                    // [chains]
  // the per-coordinate work of the new command in the same launch (null upd_vecs: a separate ppcx_update_kernel does
  // it): grid.x workgroups per chain, each runs the step redundantly and updates its share of the coordinates
  double* upd_vecs; long upd_Dpad; double* upd_t0_out;
  XchgArgs x;                   // nranks > 1: the sums are exchanged with the other ranks' state machines (pipelined rounds)
};

constexpr int kMaxShards = 16;
struct ShardSumArgs { double* bufs[kMaxShards]; int n_shards; int n; };

struct UpdateArgs {
  Dims d;
  const Cmd* cmds;              // the commands the step kernel just wrote
  double* vecs; long Dpad;
  double* draws; long draws_chain_stride;
  double* t0_out;               // [chains][nblocks_update]
};

enum AdviOp : int { ADVI_DRAW = 0, ADVI_RESET = 1, ADVI_STEP = 2 };
struct AdviArgs {
  Dims d;
  double* vecs; long Dpad;      // slot c = evaluation slot c; slot 0 also stores mu/omega/history/initial point
  double* hyper;                // slot 0 hyper vectors [V_COUNT][8]
  Cmd* cmds;                    // [n_slots]
  const double* red;            // reduced sums of slot 0 (ADVI_STEP)
  int op, n_slots, first_iter;
  double eta_scaled;
  uint32_t k0, prev_draw, draw_base;
  double* out_draws; int out_row0;   // non-null: write the draws to [row][D] instead of the evaluation slots
  double* omega_part;           // [nblocks]
};
struct AdviElboArgs { Dims d; const Cmd* cmds; const double* red; int n_slots; double* acc; const double* omega_part; int n_omega_parts; };

// the posterior-predictive draws and intervals of the K checked genes' cells (ppcx_ppc.hip, statistic in ppcx_ppc.h)
struct PpcArgs {
  Dims d;
  const double* draws;          // [n_draws][D]
  long n_draws;
  const double* exposure; const double* X;
  double truncation_compensation, p_lo, p_hi;
  uint32_t k0;
  int n_gen, resample, n_cells;
  double* ci;                   // [K*S][4] mean, sd, lower, upper
  int* counts_rng;              // [n_gen][K*S] or null
  int* scratch;                 // null: a cell's draws in LDS (grid = n_cells); else [grid][n_gen] global scratch, cells in turn
};

// streamed: the form of the kernel that reads the per-sample constants from global memory (ppcx_loglik.h; sampleE and X must
// then be readable kLdsPad entries past their ends) -- a property of the model (ppcx_model::streamed)
hipError_t launch_loglik_kernel(int CM, const LoglikArgs& a, bool streamed, hipStream_t st);
int loglik_resident_workgroups_per_cu(int CM, const Dims& d, bool streamed);   // 0: the kernel cannot be launched with this much LDS
size_t loglik_lds_bytes(const Dims& d, bool streamed);
// defined in ppcx_kernels.hip, used by the merged launch's helpers (ppcx_kernels_ls.hip) as well: the route with an exp per cell
// that the model's genes can need (GEN), and the workgroups of 256 threads of kernel f that a CU holds with lds_bytes of dynamic
// LDS each (0: the query failed)
int loglik_generic_possible(const Dims& d);
int resident_workgroups_per_cu(const void* f, size_t lds_bytes);
size_t disp_build_lds_bytes(int S);            // LDS of a workgroup of the dispersion-table kernel: a row of S counts and the node values
hipError_t launch_close_kernel(int CM, const CloseArgs& a, int nblocks, int nchains, hipStream_t st);
// pipelined rounds: the merged launch (the state machines take position 7 of the first n_srun runs of 8 x chains
// workgroups, log-likelihood range blocks everything else) and the gene kernel
// ev_start / ev_stop (both or neither): events attached to the dispatch itself (hipExtLaunchKernel) -- their elapsed time is the
// kernel's own duration, without the marker packets of a hipEventRecord on either side of the launch
hipError_t launch_ls_kernel(int CM, const LoglikArgs& a, const StepArgs& sa, int n_srun, int n_chains_total, int spec, hipStream_t st,
                            hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
int ls_resident_workgroups_per_cu(int CM, const Dims& d);
hipError_t launch_gene_kernel(int CM, const GeneArgs& a, int nblocks, int nchains, hipStream_t st);
hipError_t launch_step_kernel(const StepArgs& a, int nblocks, int nchains, hipStream_t st);
hipError_t launch_sum_shards_kernel(const ShardSumArgs& a, hipStream_t st);
hipError_t launch_update_kernel(const UpdateArgs& a, int nblocks, int nchains, hipStream_t st);
hipError_t launch_advi_kernel(const AdviArgs& a, int nblocks, hipStream_t st);
hipError_t launch_advi_elbo_kernel(const AdviElboArgs& a, hipStream_t st);
// the dispersion tables (ppcx_disp.h) of the genes in `genes` (null: genes 0 .. n_genes - 1), one workgroup per gene
hipError_t launch_disp_build_kernel(const int* counts, int G, int S, const int* genes, int n_genes, const DispFit& fit, double* table, hipStream_t st);
hipError_t launch_gather_kernel(const double* draws, long n_rows, int D, const int* cols, int n_cols, double* out, hipStream_t st);
hipError_t launch_fill_kernel(double* p, long n, double val, hipStream_t st);

// the fit summary (ppcx_summary.hip, statistics in ppcx_summary.h): columns of up to kSummaryLdsDraws draws are summarised in
// LDS (sort buffer + sequences: 128 KB at most), longer ones on a slice of global scratch per workgroup
constexpr int kSummaryLdsDraws = 8192;
constexpr int kSummaryMaxChains = 128;
struct SummaryArgs {
  const double* x;              // [n_cols][M n] the columns, chain-major (ppcx_summary_gather_kernel)
  int n_cols, M, n;
  int npad;                     // summary_npad(M, n): the sort buffer
  double* out;                  // [n_cols][SUM_FIELDS]
  double* scratch; long slice;  // null: LDS path; else [grid][slice] doubles (summary_slice_doubles)
};
int summary_npad(int M, int n);
long summary_slice_doubles(int M, int n);
size_t summary_lds_bytes(int M, int n);       // 0: the columns are too long for the LDS path
hipError_t launch_summary_gather_kernel(const double* draws, const double* lp, long rows, int D, const int* cols, int n_cols, double* out, hipStream_t st);
hipError_t launch_summary_kernel(const SummaryArgs& a, int nblocks, hipStream_t st);
// the summary of the columns `cols` (host; -1: lp) of M chains of n draws [M n][D] (device) into out [n_cols][SUM_FIELDS]
// (host), through column scratch and slices of at most scratch_bytes together (kSummaryScratchBytes in the product); synchronous
constexpr size_t kSummaryScratchBytes = (size_t)256 << 20;
hipError_t summary_columns(const double* draws, const double* lp, int M, int n, int D, int n_cols, const int* cols, double* out,
                           size_t scratch_bytes, hipStream_t st);

// the Pareto-k diagnostic of an ADVI fit (ppcx_psis.hip, statistic in ppcx_psis.h): the M + 1 largest values of a column are
// selected and sorted in LDS (kPsisMaxSel of them at most: columns of up to 1.86 million draws); columns of up to kPsisLdsDraws
// draws are staged in LDS, longer ones transformed in place in the column scratch
constexpr int kPsisLdsDraws = 4096;
constexpr int kPsisMaxSel = 4096;
constexpr size_t kPsisScratchBytes = (size_t)256 << 20;
struct PsisArgs {
  double* x;                    // [n_cols][n] the columns (ppcx_summary_gather_kernel; column -1: r); rewritten on the long path
  const double* r;              // [n] the log ratios
  const int* cols;              // [n_cols] column ids, -1: r itself
  int n_cols; long n;
  int sel_pad;                  // psis_sel_pad(n): the selection buffer
  double* out;                  // [n_cols] k-hat
};
int psis_sel_pad(long n);       // power of two >= M + 1 for n draws
hipError_t launch_psis_approx_kernel(const Dims& d, const double* sq, const double* sg, const double* hyper, double* mu, double* omega,
                                     hipStream_t st);
hipError_t launch_psis_stage_kernel(const Dims& d, const double* draws, long row0, int n_slots, double* vecs, long Dpad, Cmd* cmds,
                                    hipStream_t st);
hipError_t launch_psis_record_kernel(const Dims& d, const Cmd* cmds, const double* red, int n_slots, double* log_p, hipStream_t st);
hipError_t launch_psis_log_g_kernel(const double* draws, long rows, int D, const double* mu, const double* omega, const double* log_p,
                                    double* log_g, double* r, hipStream_t st);
hipError_t launch_psis_kernel(const PsisArgs& a, hipStream_t st);
// k-hat of the columns `cols` (host; -1: r) of draws [n][D] and r [n] (device), through column scratch of at most scratch_bytes
// per batch (kPsisScratchBytes in the product); synchronous
hipError_t psis_columns(const double* draws, const double* r, long n, int D, int n_cols, const int* cols, double* khat,
                        size_t scratch_bytes, hipStream_t st);
// PSIS-LOO per observed cell of a NUTS fit (ppcx_loo.hip, statistic in ppcx_loo.h): one workgroup per cell; the cell's ratios
// live in LDS up to kPsisLdsDraws draws, beyond that in a global scratch of at most the scratch bound per batch; the gene
// table T of a batch of genes is bounded the same way
struct LooArgs {
  const double* T = nullptr;    // [genes][C + 1][n] (ppcx_loo_table_kernel), or null: host-given columns
  const int* y = nullptr;       // [cells] the counts, an excluded cell as -(y + 1)
  const double* expo = nullptr; // [S] exposure
  const double* X = nullptr;    // [C][S] design, column-major
  int S = 1, C = 1;
  const double* cols = nullptr; // [cells][n] log-likelihood columns (testing build), instead of T
  const int* excl = nullptr;    // [cells] excluded flags of the given columns (null: none)
  const double* r_eff = nullptr;   // [cells] relative efficiencies (null: 1)
  const double* lr = nullptr;   // [n] log_p - log_g of an ADVI fit's draws: the approximate-posterior statistic (ppcx_loo_ap.h)
  long n = 0;                   // draws
  int cell0 = 0, n_cells = 0;   // first cell of the launch; cells of the table / columns
  double* scratch = nullptr;    // [launch's cells][slice] the long path's arrays, `slice` doubles per cell as the statistic's kernel
                                //  lays them out (set per batch by cells_in_batches, ppcx_loo_dev.h)
  int sel_pad = 0;              // loo_sel_pad: the selection buffer
  double* out = nullptr;        // [cells][kLooFields], or [cells][kLooMcseFields] (ppcx_fit_loo_mcse)
};
int loo_sel_pad(long n, double r_eff_min);     // power of two >= M + 1 for n draws at the smallest r_eff
hipError_t launch_loo_table_kernel(const double* draws, long n_draws, const Dims& d, const int* genes, int n_genes, double* T,
                                   hipStream_t st);    // T[g][c][draw] of the genes (device ids), ppcx_loo.hip
// These cells of this fit: what every per-cell driver below receives (ppcx_fit_api.hip loo_prepare fills it). The cells are those
// of genes[0 .. n_genes), S each, gene-major.
struct FitCells {
  const double* draws = nullptr;   // [n][D] (device)
  long n = 0;                      // draws = chains n_keep
  int chains = 0, n_keep = 0;
  Dims d{};
  const double* expo = nullptr;    // [S] (device)
  const double* X = nullptr;       // [C][S] (device)
  int n_genes = 0;
  const int* genes = nullptr;      // [n_genes] (host)
  const int* yenc = nullptr;       // [cells] the counts, an excluded cell as -(y + 1) (host)
  const double* r_eff = nullptr;   // [cells] (host) or null: all 1
  double r_eff_min = 1.0;          // the smallest r_eff (1 without r_eff)
  const double* log_ratio = nullptr;   // [n] (device) log_p - log_g of an ADVI fit, or null: the draws are the posterior's
};
// The driver of ppcx_fit_ppc: the table, then one wavefront per cell up to 4096 predictive draws per cell, one workgroup per cell
// beyond. Of `a` the inputs (device) are the caller's, ci / counts_rng / scratch the driver's own; ci [n_cells][4] and counts_rng
// [n_gen][n_cells] (or null) are host; kernel_ms: table + kernel by HIP events, left alone where there are none. Synchronous.
hipError_t ppc_fit(PpcArgs a, double* ci, int32_t* counts_rng, float* kernel_ms, hipStream_t st);
// Host-given log-likelihood columns in place of a fit's cells (testing build): cols [n_cols][n], n = chains n_keep where the
// statistic needs chains
struct GivenCells {
  const double* cols = nullptr; long n = 0; int n_cols = 0;
  int chains = 0, n_keep = 0;
  const int* excl = nullptr;       // [n_cols] excluded flags or null
  const double* r_eff = nullptr; double r_eff_min = 1.0;
  const double* log_ratio = nullptr;   // [n] (host) log ratios of the draws, or null
};
// The drivers below walk the cells through for_gene_batches / for_given_columns and launch through cells_in_batches
// (ppcx_loo_dev.h: LDS against scratch, the kernel's instantiation and its dynamic LDS in one place); out is host, scratch_bytes
// bounds the gene table of a batch and the cells' scratch of a launch alike (kPsisScratchBytes in the product). Synchronous.
// LOO: fields = kLooFields, or kLooMcseFields for mcse_elpd_loo and n_eff as well (out holds that many per cell; the first four
// are the same bits). With log_ratio (an ADVI fit; kLooFields only) the approximate-posterior statistic of ppcx_loo_ap.h: ratios,
// log-likelihoods and log weights (24 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond that in the scratch
hipError_t loo_fit_cells(const FitCells& fc, int fields, double* out, size_t scratch_bytes, hipStream_t st);
hipError_t loo_columns(const GivenCells& gc, int fields, double* out, size_t scratch_bytes, hipStream_t st);
// the log-likelihood matrix of the cells, [n][cells]
hipError_t loo_fit_log_lik(const FitCells& fc, double* out, size_t scratch_bytes, hipStream_t st);
// The leave-one-out predictive interval and LOO-PIT of the same cells (ppcx_loo_predict.hip, statistic in ppcx_loo_predict.h): one
// workgroup per cell; ratios, weights and predictive counts (20 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond that in
// the scratch. tc: truncation compensation of the predictive draws; k0 = seed32(seed). out [cells][kLooPredictFields]. With
// log_ratio the weights are those of ppcx_loo_ap.h
hipError_t loo_predict_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, uint32_t k0, double* out,
                                 size_t scratch_bytes, hipStream_t st);
// ... of given columns with predictive counts x [n_cols][n] and observed counts y [n_cols]
hipError_t loo_predict_columns(const GivenCells& gc, const int* x, const int* y, double p_lo, double p_hi, double* out,
                               size_t scratch_bytes, hipStream_t st);
// The exact posterior-predictive tails and interval of the same cells (ppcx_ppc_exact.hip, statistic in ppcx_ppc_exact.h): one
// workgroup per cell; (eta, ln phi) of the draws (16 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond that in the scratch.
// tc: truncation compensation. out [cells][kPpcExactFields]. Of `fc` neither r_eff nor log_ratio is used: NUTS, ADVI and
// given-draws fits alike.
hipError_t ppc_exact_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, double* out, size_t scratch_bytes,
                               hipStream_t st);
// ... of given columns: gc.cols the linear predictors [n_cols][n], sigma_raw [n_cols][n], y [n_cols] the observed counts
hipError_t ppc_exact_columns(const GivenCells& gc, const double* sigma_raw, const int* y, double tc, double p_lo, double p_hi,
                             double* out, size_t scratch_bytes, hipStream_t st);
// The exact leave-one-out predictive tails and interval of the same cells (ppcx_loo_exact.hip, statistic in ppcx_loo_exact.h): one
// workgroup per cell; ratio / eta, weight and ln phi of the draws (24 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond
// that in the scratch. tc: truncation compensation. out [cells][kLooExactFields]. With log_ratio the weights are those of
// ppcx_loo_ap.h
hipError_t loo_exact_fit_cells(const FitCells& fc, double tc, double p_lo, double p_hi, double* out, size_t scratch_bytes,
                               hipStream_t st);
// ... of given columns: gc.cols the log-likelihoods [n_cols][n], eta and sigma_raw [n_cols][n], y [n_cols] the observed counts
hipError_t loo_exact_columns(const GivenCells& gc, const double* eta, const double* sigma_raw, const int* y, double tc, double p_lo,
                             double p_hi, double* out, size_t scratch_bytes, hipStream_t st);
// Gene-local moment matching of the cells whose PSIS-LOO k-hat exceeds k_threshold (ppcx_loo_mm.hip, statistic in
// ppcx_loo_mm.h): ppcx_loo_kernel over the cells (launch_loo_kernel, ppcx_loo.hip: `n_blocks` cells from a.cell0, fields as
// loo_fit_cells), then one workgroup per cell; a candidate's ratios, the log weights and the local density at the original draws
// (24 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond that in the scratch. NUTS fits (fc.log_ratio null).
// out [cells][loo_mm_fields(C)]
hipError_t launch_loo_kernel(const LooArgs& a, int fields, int n_blocks, hipStream_t st);
hipError_t loo_mm_fit_cells(const FitCells& fc, double k_threshold, int max_iters, double* out, size_t scratch_bytes, hipStream_t st);
// The exact leave-one-out predictive under the matched weights (ppcx_loo_mm_exact.hip, statistic in ppcx_loo_mm_exact.h): per batch
// of cells the two kernels above into a device record, then one workgroup per cell; ratio / eta, weight and ln phi of the draws
// (24 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond that in the scratch. out [cells][loo_mm_exact_fields(C)]
hipError_t loo_mm_exact_fit_cells(const FitCells& fc, double k_threshold, int max_iters, double tc, double p_lo, double p_hi, double* out,
                                  size_t scratch_bytes, hipStream_t st);
// The split transformation of the matching (ppcx_loo_mm_split.hip, statistic in ppcx_loo_mm_split.h): per batch of cells the
// matching's two kernels into a device record, then one workgroup per cell; ratio / eta, weight and ll_x / ln phi of the draws
// (24 bytes per draw) in LDS up to kPsisLdsDraws draws, beyond that in the scratch. predictive false: the elpd form, out
// [cells][loo_mm_split_fields(C)] (tc, p_lo, p_hi are not read); true: the exact predictive, out [cells][loo_mm_exact_split_fields(C)]
hipError_t loo_mm_split_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool predictive, double tc, double p_lo,
                                  double p_hi, double* out, size_t scratch_bytes, hipStream_t st);
// The matching with the covariance step as its third candidate (ppcx_loo_mm_cov.hip, statistic in ppcx_loo_mm_cov.h):
// ppcx_loo_kernel over the cells, then one workgroup per cell with the affine state in static LDS; the same three arrays of n
// doubles as loo_mm_fit_cells. split: the split transformation follows in the same workgroup. out [cells][loo_mm_cov_fields(C)]
hipError_t loo_mm_cov_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool split, double* out, size_t scratch_bytes,
                                hipStream_t st);
// The exact predictive under the weights of that matching (ppcx_loo_mm_cov_exact.hip, statistic in ppcx_loo_mm_cov_exact.h): per
// batch of cells ppcx_loo_kernel and the non-split ppcx_loo_mm_cov_kernel into a device record and the accumulated inverse beside
// it, then one workgroup per cell with the states in static LDS; the same three arrays of n doubles. split: under the split
// weights. out [cells][loo_mm_cov_exact_fields(C)]
hipError_t loo_mm_cov_exact_fit_cells(const FitCells& fc, double k_threshold, int max_iters, bool split, double tc, double p_lo, double p_hi,
                                      double* out, size_t scratch_bytes, hipStream_t st);
// The relative efficiency of the same cells (ppcx_reff.hip, statistic in ppcx_reff.h): one workgroup per cell; the split values
// (8 bytes each) in LDS for fits of up to kPsisLdsDraws draws, beyond that in the scratch. Of `l` it uses T / y / expo / X / S / C
// or cols, n = chains n_keep, cell0, n_cells, scratch ([launch's cells][2 chains (n_keep / 2)]) and out ([cells], one value
// each). At most kSummaryMaxChains chains.
struct ReffArgs { LooArgs l; int chains = 0, n_keep = 0; };
hipError_t reff_fit_cells(const FitCells& fc, double* out, size_t scratch_bytes, hipStream_t st);
hipError_t reff_columns(const GivenCells& gc, double* out, size_t scratch_bytes, hipStream_t st);
hipError_t launch_xchg_abort_kernel(const XchgArgs& x, hipStream_t st);      // tells every peer that this rank has left the fit

}  // namespace ppcx
