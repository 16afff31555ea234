/* ppcx_testing.h -- entry points that exist only in the TESTING build of the library (-DPPCX_TESTING:
 * tests/libppcx_testing.so, built by __graft_entry__.build() next to the product). They are test infrastructure
 * (fault injection, forcing a cell path, a stand-in provider of the nccl* entry points, kernel-level timing); the
 * shipped ppcseq_amd/libppcx.so neither exports them nor contains the code behind them. */
#ifndef PPCX_TESTING_H
#define PPCX_TESTING_H
#include "../../include/ppcx.h"
#ifdef __cplusplus
extern "C" {
#endif
/* keys: "fail_at_round" (a rank of a gene-sharded run reports a failure once it has issued that many rounds),
 * "fail_rank" (-1: every rank), "force_generic" (genes with slopes form eta per cell even in a factor design; applies to
 * models created afterwards),
 * "slope_cost_permille", "trim_slack_permille", "trim_extra_passes" (the launch plan's cost of a pass with slopes / slack of
 * a chain group's trimmed launch, per mille / passes per wavefront of such a launch beyond the fewest possible; -1 or 0:
 * built-in; plans made afterwards),
 * "psis_slots", "psis_scratch_bytes" (the Pareto-k diagnostic: draws per launch of the log_p evaluation, bound of the column
 * scratch per batch; 0: built-in),
 * "loo_scratch_bytes" (PSIS-LOO: bound of the gene table, of the long columns' scratch and of the exported log-likelihood
 * block per batch; 0: built-in). */
PPCX_API int ppcx_testing_set(const char* key, long long value);
/* path of a shared object that provides ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce /
 * ncclGetErrorString instead of librccl (before the first communicator is created) */
PPCX_API int ppcx_testing_set_nccl_provider(const char* path);
enum { PPCX_BENCH_LOGLIK = 0, PPCX_BENCH_CLOSE = 1, PPCX_BENCH_LOGLIK_CLOSE = 2, PPCX_BENCH_STEP = 3, PPCX_BENCH_UPDATE = 4,
       PPCX_BENCH_STEP_REDUCE = 5, PPCX_BENCH_STEP_ADVANCE = 6, PPCX_BENCH_STEP_UPDATE = 7,
       PPCX_BENCH_GENE = 8,           /* the gene kernel of a pipelined round on a leaf command (apply + close + anticipate) */
       PPCX_BENCH_GENE_NO_PROP = 9,   /* the same without the proposal copy: what an index-based proposal store would save */
       PPCX_BENCH_GENE_NO_SPEC = 10,  /* ... without the anticipated constants */
       PPCX_BENCH_GENE_UPDATE_ONLY = 11,  /* ... the command's coordinate work only (no close) */
       PPCX_BENCH_GENE_NEW_TRANSITION = 12 };  /* the first leaf of a transition: fresh momenta for every coordinate */
PPCX_API int ppcx_testing_bench_kernel(ppcx_model* m, int which, int nchains, int warm_rounds, int reps, int n_merge,
                                       double* ms_per_launch, int* cmd_type);
/* mean microseconds per round of a chain's state machine by phase since the last call (ppcx_fit_nuts.hip) */
PPCX_API int ppcx_testing_sm_trace(double* out6);
/* The device's scalar building blocks element by element (ppcx_testing_math.hip): out0[i], out1[i] of function `fn` at a[i],
 * b[i], y[i]; the log tables are in LDS, the cells run with their gfx950 assembly.
 *   FAST_RCP / FAST_LOG / FAST_EXP / TABLE_LOG / WINDOW_LOG (ppcx_math.h): out0 = f(a)
 *   STIRLING_TAILS: out0, out1 = lg_tail, dg_tail of r = a          STIRLING_EXCESS: dlt, dps of phi = a, ln phi = b, any_small = y
 *   LOG_ERFC_RATIO: log erfc(a), exp(-a^2)/erfc(a)
 *   CELL / CELL_WIN (ppcx_model.h cell_eval / cell_eval_win with one = 1): ln w, 1/w of w = fma(a, b, 1), count y
 *   CELL_Y / CELL_WIN_Y: the same cells' y ln w and y / w accumulations
 *   the posterior-predictive sampler's own functions (ppcx_math.h, the __HIP_DEVICE_COMPILE__ branch):
 *   SINCOS_2PI: out0, out1 = sin, cos of 2 pi a         LGAMMA_INT1: out0 = lgamma_int1(a)
 *   RNG_EXP: out0 = rng_exp(a)                          RNG_DIV: out0 = rng_div(a, b)
 *   NB2_TAILS (ppcx_nbcdf.h nb2_log_tails): out0, out1 = P(X <= y), P(X >= y) of X ~ NB(mean e^a, size b) */
enum { PPCX_MATH_FAST_RCP = 0, PPCX_MATH_FAST_LOG = 1, PPCX_MATH_FAST_EXP = 2, PPCX_MATH_TABLE_LOG = 3, PPCX_MATH_WINDOW_LOG = 4,
       PPCX_MATH_STIRLING_TAILS = 5, PPCX_MATH_STIRLING_EXCESS = 6, PPCX_MATH_LOG_ERFC_RATIO = 7, PPCX_MATH_CELL = 8,
       PPCX_MATH_CELL_WIN = 9, PPCX_MATH_CELL_Y = 10, PPCX_MATH_CELL_WIN_Y = 11, PPCX_MATH_SINCOS_2PI = 12, PPCX_MATH_LGAMMA_INT1 = 13,
       PPCX_MATH_RNG_EXP = 14, PPCX_MATH_RNG_DIV = 15, PPCX_MATH_NB2_TAILS = 16, PPCX_MATH_COUNT = 17 };
PPCX_API int ppcx_testing_eval_math(int fn, int n, const double* a, const double* b, const int* y, double* out0, double* out1);
/* the model's dispersion tables as the device built them: G x 768 doubles (ppcx_disp.h layout) */
PPCX_API int ppcx_testing_get_disp_table(ppcx_model* m, double* out);
/* The Pareto-k kernel of ppcx_fit_psis on host-given values, on the current device (ppcx_psis.hip): lr [n] the log ratios,
 * cols [n][n_cols] row-major parameter draws; khat [n_cols + 1]: the k-hat of 1/2 log1p(cols[:, i]^2) + lr for i < n_cols,
 * then that of lr itself. */
PPCX_API int ppcx_testing_psis(int n, int n_cols, const double* lr, const double* cols, double* khat);
/* The PSIS-LOO kernel of ppcx_fit_loo on host-given log-likelihood columns, on the current device (ppcx_loo.hip): ll [n_cols][n]
 * (column-major: a cell's n draws contiguous), excluded NULL or [n_cols] flags, r_eff NULL or [n_cols]; out [n_cols][4]. */
PPCX_API int ppcx_testing_loo(int n, int n_cols, const double* ll, const int32_t* excluded, const double* r_eff, double* out);
/* The same kernel as ppcx_fit_loo_mcse runs it: out [n_cols][6], the four fields above (the same bits), mcse_elpd_loo, n_eff. */
PPCX_API int ppcx_testing_loo_mcse(int n, int n_cols, const double* ll, const int32_t* excluded, const double* r_eff, double* out);
/* The kernel of ppcx_fit_loo_predict on host-given columns, on the current device (ppcx_loo_predict.hip): ll [n_cols][n]
 * log-likelihoods and x [n_cols][n] predictive counts (>= 0; a cell's n draws contiguous), y [n_cols] the observed counts, excluded
 * NULL or [n_cols] flags, r_eff NULL or [n_cols]; out [n_cols][6]: mean, lower, upper, pit_lt, pit_le, khat. */
PPCX_API int ppcx_testing_loo_predict(const double* ll, const int32_t* x, int n, int n_cols, const int32_t* y, const int32_t* excluded,
                                      const double* r_eff, double p_lo, double p_hi, double* out);
/* The kernels of ppcx_fit_loo_approx and ppcx_fit_loo_predict_approx on host-given columns (ppcx_loo_ap.h): as the two above
 * with log_ratio [n], the draws' log_p - log_g, and r_eff = 1. */
PPCX_API int ppcx_testing_loo_approx(int n, int n_cols, const double* ll, const double* log_ratio, const int32_t* excluded, double* out);
PPCX_API int ppcx_testing_loo_predict_approx(const double* ll, const double* log_ratio, const int32_t* x, int n, int n_cols,
                                             const int32_t* y, const int32_t* excluded, double p_lo, double p_hi, double* out);
/* The kernel of ppcx_fit_relative_eff on host-given log-likelihood columns, on the current device (ppcx_reff.hip): ll
 * [n_cols][chains n] (a cell's draws contiguous, chain-major), out [n_cols]. */
PPCX_API int ppcx_testing_relative_eff(int chains, int n, int n_cols, const double* ll, double* out);
/* The kernel of ppcx_fit_ppc_exact on host-given columns, on the current device (ppcx_ppc_exact.hip): eta [n_cols][n] the linear
 * predictors and sigma_raw [n_cols][n] (a cell's n draws contiguous), y [n_cols] the observed counts (>= 0), excluded NULL or
 * [n_cols] flags; out [n_cols][9]: mean, sd, p_le, p_ge, lower, upper, y, excluded, outside. */
PPCX_API int ppcx_testing_ppc_exact(int n, int n_cols, const double* eta, const double* sigma_raw, const int32_t* y,
                                    const int32_t* excluded, double truncation_compensation, double p_lo, double p_hi, double* out);
/* The kernel of ppcx_fit_loo_predict_exact on host-given columns, on the current device (ppcx_loo_exact.hip): ll, eta and sigma_raw
 * [n_cols][n] (a cell's n draws contiguous; ll need not be the log-pmf of y at eta and sigma_raw), y [n_cols] the observed counts
 * (>= 0), excluded NULL or [n_cols] flags, r_eff NULL or [n_cols]; log_ratio NULL, or [n] the draws' log_p - log_g: the kernel as
 * ppcx_fit_loo_predict_exact_approx runs it (r_eff then NULL). Probabilities and truncation compensation as the entry points
 * check them. out [n_cols][10]: mean, sd, p_le, p_ge, lower, upper, y, excluded, outside, khat. */
PPCX_API int ppcx_testing_loo_exact(int n, int n_cols, const double* ll, const double* eta, const double* sigma_raw, const int32_t* y,
                                    const int32_t* excluded, const double* r_eff, const double* log_ratio,
                                    double truncation_compensation, double p_lo, double p_hi, double* out);
/* A fit over host-given draws [n_keep][D] and host-given log ratios log_ratio [n_keep] (log_p - log_g, -Inf allowed) that the
 * _approx entries accept (ppcx_fit_loo_approx, ppcx_fit_loo_moment_match_approx, ...): designed draw sets reach their kernels this
 * way. The fit counts as an ADVI fit of one chain; its approximation (ppcx_fit_get_approximation) is zeros and means nothing. */
PPCX_API int ppcx_testing_fit_from_draws_approx(ppcx_model* m, int n_keep, const double* draws, const double* log_ratio, ppcx_fit** out);
#ifdef __cplusplus
}
#endif
#endif
