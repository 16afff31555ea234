/* ppcx.h -- C ABI of the MI355X-native posterior-predictive-check engine for ppcseq's
 * negative-binomial hierarchical model.
 *
 * This is the drop-in boundary for the ONE hot path of stemangiola/ppcseq: what
 * `do_inference()` (R/utilities.R:1321-1547) obtains today from
 *     rstan::sampling(stanmodels$negBinomial_MPI, ...)            R/utilities.R:1497-1512
 *     rstan::summary(fit, "counts_rng", prob = c(p, 1-p))         R/utilities.R:685-703
 *     rstan::extract(fit, "lambda_log_param" / "sigma_raw")       R/utilities.R:738,743
 *     rstan::summary(fit, "alpha_sub_1") (slope)                  R/utilities.R:1531,1250-1263
 * whose model object is registered by src/RcppExports.cpp:15-25 / R/stanmodels.R:7-25.
 * The Stan data block (inst/stan/negBinomial_MPI.stan:142-173) carries CPU-threading packing
 * (counts_package, G_ind, symbol_end ...); this ABI takes the LOGICAL inputs instead and the
 * R shim in INTEGRATION.md undoes the packing.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; every function returns a status
 * (0 = ok, < 0 = error class, message via ppcx_last_error()); the caller owns every buffer it
 * passes, the library never keeps a caller pointer after return; device memory is internal.
 * One call at a time per handle; different handles may be used from different threads.
 */
#ifndef PPCX_H
#define PPCX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define PPCX_API __attribute__((visibility("default")))
#else
#define PPCX_API
#endif

#define PPCX_OK 0
#define PPCX_ERR_ARG (-1)       /* invalid argument                                   */
#define PPCX_ERR_HIP (-2)       /* HIP runtime error (message has hipGetErrorString)  */
#define PPCX_ERR_INIT (-3)      /* no finite initial point after 100 attempts (Stan)  */
#define PPCX_ERR_STEPSIZE (-4)  /* step-size heuristic left (0, 1e7) (Stan)           */
#define PPCX_ERR_STALL (-5)     /* launch budget exhausted (internal guard)           */
#define PPCX_ERR_LIMIT (-6)     /* size limit of this build                           */
#define PPCX_ERR_CANCELLED (-7) /* the caller's progress callback ended the fit       */

typedef struct ppcx_model ppcx_model;
typedef struct ppcx_fit ppcx_fit;

/* ABI version: bumped whenever the layout or meaning of an argument changes. 100 = round 1; 200 = round 2 (dims[15] /
 * reals[6] / counts_rng + errbuf + errlen of ppcx_do_inference_C, ppcx_model_set_launch's second argument = workgroups);
 * 300 = this one: ppcx_do_inference_C takes the version its caller was written for as dims[0], so that a shim built for
 * another layout gets PPCX_ERR_ARG instead of reading past its arrays.                                                */
#define PPCX_VERSION 400
PPCX_API int ppcx_version(void);
PPCX_API int ppcx_device_count(void);
/* free and total memory of a device in bytes (what R/methods.R:178-195 asks the host about before keeping all draws) */
PPCX_API int ppcx_device_memory(int device, unsigned long long* free_bytes, unsigned long long* total_bytes);
PPCX_API const char* ppcx_last_error(void);

/* --- model = Stan data block (inst/stan/negBinomial_MPI.stan:142-173), logical form -------------
 * counts : G x S int32, gene-major (sample index fastest); genes 0..K-1 are the checked ones
 *          (how_many_to_check, R/utilities.R:1364-1368; G order R/utilities.R:949-952)
 * X      : S x C doubles, column-major (R model.matrix, R/utilities.R:887-900)
 * exposure_rate : S (R/utilities.R:1466-1473);  lambda_mu_mu = 5.612671 (R/methods.R:218)
 * excl   : n_excl cell ids g*S+s, 0-based (to_exclude, R/utilities.R:321-359 / .stan:105-115)      */
PPCX_API int ppcx_model_create(int device, int G, int S, int C, int K, const int32_t* counts, const double* X,
                      const double* exposure_rate, double lambda_mu_mu, int n_excl, const int32_t* excl,
                      ppcx_model** out);
/* ... with a choice of where the log-likelihood kernel keeps the per-sample constants (exp(exposure_s) and the design's slope
 * columns: S * C doubles; S * (2 + C) for a design without the column of ones). In LDS they share a compute unit's 160 KB with
 * 20 KB of tables, which bounds S (8 704 at C = 2, 2 176 at C = 8, 1 088 at C = 16); streamed, the kernel reads them from global
 * memory and the bound is the dispersion-table kernel's row of counts, S <= 39 552 (PPCX_ERR_LIMIT beyond).
 *   PPCX_PER_SAMPLE_LDS    exactly ppcx_model_create, its refusals included
 *   PPCX_PER_SAMPLE_STREAM always streamed
 *   PPCX_PER_SAMPLE_AUTO   LDS where ppcx_model_create accepts the model (the same model, bit for bit), streamed where it
 *                          refuses it for LDS
 * A streamed model runs the three-launch round (ppcx_model_get_rounds says so; ppcx_fit_nuts_xchg refuses it); the gene-shard
 * constructors stay on LDS. The refusals of more than 16 columns, and of a continuous covariate or a missing column of ones
 * among more than 8, hold for every value.                                                                                  */
#define PPCX_PER_SAMPLE_LDS 0
#define PPCX_PER_SAMPLE_STREAM 1
#define PPCX_PER_SAMPLE_AUTO 2
PPCX_API int ppcx_model_create_ex(int device, int G, int S, int C, int K, const int32_t* counts, const double* X,
                      const double* exposure_rate, double lambda_mu_mu, int n_excl, const int32_t* excl,
                      int per_sample, ppcx_model** out);
PPCX_API int ppcx_model_get_per_sample(const ppcx_model* m, int* streamed);   /* 1: the model streams them, 0: LDS */
PPCX_API int ppcx_model_set_exclusions(ppcx_model* m, int n_excl, const int32_t* excl);   /* pass 2 of R/methods.R:320-342 */
PPCX_API int ppcx_model_set_launch(ppcx_model* m, int lanes_per_gene, int workgroups); /* 0 = automatic; lanes: power of two <= 64 */
PPCX_API int ppcx_model_get_launch(const ppcx_model* m, int* lanes_per_gene, int* nblocks);
/* round structure of the NUTS fits of this model. pipelined: -1 = two launches per leapfrog wherever the model allows it
   (default), 0 = always the three-launch round, -2 = leave the setting as it is; stream_groups: 0 = by the number of chains
   (default), n = the chains run in n groups on their own streams, -1 = leave the setting as it is. A chain's draws do not
   depend on stream_groups. The initial values come from the environment variables PPCX_PIPELINE / PPCX_STREAM_GROUPS, read
   once when the model is created. */
PPCX_API int ppcx_model_set_rounds(ppcx_model* m, int pipelined, int stream_groups);
/* Progress of a running NUTS fit (rstan prints the chains' iterations; a fit of minutes need not be silent, and a chain that left
   the reference's 150 warm-up iterations with a very small step size -- every transition at the maximum tree depth, DESIGN.md
   section 4 -- shows up here as one chain still running long after the others): fn(user, first_chain_of_the_group,
   chains_in_the_group, chains_done, leapfrog_rounds_issued, seconds) is called from the thread that pumps the group's launches,
   at most every `every_seconds` and once when the group is done. NULL switches it off (default).
   The callback's return value is the caller's budget: nonzero ends the fit -- no further rounds are issued for the group, the
   other groups end at their next report, a gene-sharded run takes its peers along as after any failure -- and the fit call
   returns PPCX_ERR_CANCELLED with nothing to free; the model stays usable. */
typedef int (*ppcx_progress_fn)(void* user, int first_chain, int chains, int chains_done, long long rounds, double seconds);
PPCX_API int ppcx_model_set_progress(ppcx_model* m, ppcx_progress_fn fn, void* user, double every_seconds);
/* what a fit of `nchains` chains of this model runs: pipelined = 1 (two launches per leapfrog: any model with X[,1] = 1 whose
   slope columns are 0 / 1 indicators -- `~ 1`, `~ Label`, formulas of factors) or 0 (three launches: continuous covariates),
   and the number of chain groups */
PPCX_API int ppcx_model_get_rounds(const ppcx_model* m, int nchains, int* pipelined, int* stream_groups);
/* diagnostic: the log-likelihood launch planned for `nchains` chains -- lanes per gene, workgroups per chain and the
   gene-order positions bounds[0 .. 4 * workgroups_per_chain] delimiting the wavefronts' ranges (NULL to skip).
   nchains < 0: the launch of -nchains chains of one of SEVERAL chain groups, which leaves the workgroup slots it cannot use
   to the other groups' launches, at the lanes per gene in force (of the last fit, plan or ppcx_model_set_launch) */
PPCX_API int ppcx_model_get_plan(ppcx_model* m, int nchains, int* lanes_per_gene, int* workgroups_per_chain, int* bounds, int cap);
PPCX_API int ppcx_model_dim(const ppcx_model* m);          /* D = 2G + K*max(C-1,1) + 6 */
PPCX_API void ppcx_model_destroy(ppcx_model* m);

/* log_prob + gradient on the unconstrained scale, Stan parameter order (.stan:183-197), Jacobians
 * included, `~` constants dropped, neg_binomial_2_log_lpmf constants kept (what NUTS integrates).
 * u, grad: n_points x D ; lp: n_points.                                                             */
PPCX_API int ppcx_log_prob_grad(ppcx_model* m, int n_points, const double* u, double* lp, double* grad);

/* --- NUTS = rstan::sampling call of R/utilities.R:1497-1512 ------------------------------------- */
typedef struct {
  int chains, iter, warmup;          /* iter includes warmup (Stan convention)                     */
  unsigned long long seed;
  double adapt_delta;                /* 0.8  */
  int max_treedepth;                 /* 10   */
  double init_radius;                /* 2    (init = "random")                                     */
  double stepsize0;                  /* 1    */
  int init_buffer, term_buffer, window;   /* 75, 50, 25                                            */
  int chain_id_offset;               /* global id of chain 0 of this call (multi-GPU: rank*chains)  */
} ppcx_nuts_config;
PPCX_API void ppcx_nuts_config_default(ppcx_nuts_config* cfg);

PPCX_API int ppcx_fit_nuts(ppcx_model* m, const ppcx_nuts_config* cfg, ppcx_fit** out);
PPCX_API int ppcx_fit_info(const ppcx_fit* f, int* chains, int* n_keep, int* D, int* iter);
/* a fit holding draws produced elsewhere, [chains][n_keep][D] unconstrained (the host layer gathers the chains of other
 * ranks): ppcx_fit_ppc / ppcx_fit_get_columns then see the pooled posterior, as rstan::summary does over merged chains
 * (R/utilities.R:685-703, :1500-1501)                                                                                    */
PPCX_API int ppcx_fit_from_draws(ppcx_model* m, int chains, int n_keep, const double* draws, ppcx_fit** out);
/* kept draws, unconstrained, [chains][n_keep][D] */
PPCX_API int ppcx_fit_get_draws(ppcx_fit* f, double* out);
/* selected columns of the kept draws, [chains*n_keep][n_cols] */
PPCX_API int ppcx_fit_get_columns(ppcx_fit* f, int n_cols, const int32_t* cols, double* out);
/* Per-column summary of the kept draws (rstan::monitor, and the checks rstan::sampling runs after a fit: R-hat > 1.05, bulk or
 * tail ESS < 100 x chains). out[i][PPCX_SUMMARY_FIELDS] for column cols[i] (-1 = lp__): mean, sd (ddof 1), q05, q50, q95 (type 7)
 * over all draws; the rank-normalised split R-hat (the larger of the bulk and the folded one); the bulk ESS of the rank-normalised
 * split chains; the tail ESS (the smaller of those of 1[x <= q05] and 1[x <= q95]) -- Vehtari, Gelman, Simpson, Carpenter, Buerkner
 * (2021). A column with a non-finite draw is NaN throughout; one without variance, or with fewer than 4 draws per chain, has NaN
 * R-hat and ESS. NUTS fits of every entry point and ppcx_fit_from_draws fits (which hold no lp__); an ADVI fit, a column out of
 * range, -1 on a fit without lp__ or more than 128 chains: PPCX_ERR_ARG (PPCX_ERR_LIMIT for the chains). Synchronous on the
 * model's stream; the same bits on every call.                                                                              */
#define PPCX_SUMMARY_FIELDS 8   /* mean, sd, q05, q50, q95, rhat, ess_bulk, ess_tail */
PPCX_API int ppcx_fit_summary(ppcx_fit* f, int n_cols, const int32_t* cols, double* out);
/* The Pareto-k diagnostic of an ADVI fit (what rstan::vb reports from rstan 2.21 on: Pareto-smoothed importance sampling on the
 * log ratios log_p - log_g of the output draws, and a khat column in its summary). Only fits of ppcx_fit_advi /
 * ppcx_fit_advi_iterative; a NUTS fit, a ppcx_fit_from_draws fit or a column out of range: PPCX_ERR_ARG.
 *   ppcx_fit_get_approximation  mu and omega (log sd) of the fitted mean-field approximation, D values each (either may be NULL).
 *   ppcx_fit_get_log_ratios     log_p (the model's log density, without constants, as the ELBO evaluates it; under the model's
 *                               exclusions when first asked) and log_g = -1/2 sum_d ((theta_d - mu_d) exp(-omega_d))^2 (Stan's
 *                               calc_log_g: the terms common to every draw cancel) at each kept draw, n_keep values each.
 *                               Evaluated once per fit, on the first call of this or ppcx_fit_psis, and kept on the device.
 *   ppcx_fit_psis               khat[i] of column cols[i]: -1 = the log ratios r themselves (the overall k-hat rstan warns on:
 *                               > 0.7 resampling unreliable, > 1 disabled), d = 1/2 log1p(theta_d^2) + r (rstan's per-parameter
 *                               khat). r = -Inf where log_p is not finite: such draws take no part. Fewer than 5 tail draws or a
 *                               constant tail: +Inf; a non-finite theta_d: NaN. Synchronous on the model's stream; the same
 *                               bits on every call. More than 1.86 million kept draws: PPCX_ERR_LIMIT.                      */
PPCX_API int ppcx_fit_get_approximation(ppcx_fit* f, double* mu, double* omega);
PPCX_API int ppcx_fit_get_log_ratios(ppcx_fit* f, double* log_p, double* log_g);
PPCX_API int ppcx_fit_psis(ppcx_fit* f, int n_cols, const int32_t* cols, double* khat);
/* PSIS-LOO per observed cell of a NUTS fit (what rstan::loo(fit) / loo::loo(log_lik, r_eff) report per observation; the
 * Monte-Carlo standard error and the effective sample size through ppcx_fit_loo_mcse). Every count is one observation: cell (g, s) of a gene g in genes[0 .. n_genes) and a sample s. NUTS fits of every
 * entry point and ppcx_fit_from_draws fits; an ADVI fit, a gene out of range or a bad r_eff: PPCX_ERR_ARG. Synchronous on the
 * model's stream; the same bits on every call, whatever other genes are requested.
 *   ppcx_fit_get_log_lik  log_lik = neg_binomial_2_log_lpmf(y | exposure_s + X_s alpha_g, exp(-sigma_raw_g)) with every constant
 *                         kept, out [chains][n_keep][n_genes][S]; cells excluded by the model hold theirs too.
 *   ppcx_fit_loo          out [n_genes][S][PPCX_LOO_FIELDS]: elpd_loo, p_loo, looic, khat of loo's PSIS on r = -log_lik over
 *                         the kept draws, tail length ceil(min(0.2 N, 3 sqrt(N / r_eff))); r_eff NULL (all 1) or [n_genes][S],
 *                         each finite and > 0. A cell excluded by the model at the time of the call is already held out:
 *                         elpd_loo = lpd (its exact held-out predictive density), p_loo = 0, khat = NaN. A NaN log_lik or one of
 *                         -Inf: the cell is NaN; fewer than 5 tail draws or a constant tail: khat = +Inf and raw weights.
 *                         The log-likelihood matrix is never materialised. A tail of more than 4 095 draws (1.86 million
 *                         kept draws at r_eff = 1, fewer at smaller r_eff): PPCX_ERR_LIMIT.                                  */
#define PPCX_LOO_FIELDS 4       /* elpd_loo, p_loo, looic, khat */
PPCX_API int ppcx_fit_get_log_lik(ppcx_fit* f, int n_genes, const int32_t* genes, double* out);
PPCX_API int ppcx_fit_loo(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double* out);
/* ppcx_fit_loo with how far each cell's elpd_loo can be trusted once its khat is acceptable: loo::loo's pointwise mcse_elpd_loo
 * (its deterministic form on 1 000 Blom scores) and psis_n_eff, restated from the published package. Fits, genes, r_eff, refusals
 * and limits as ppcx_fit_loo. out [n_genes][S][PPCX_LOO_MCSE_FIELDS]: the four fields of ppcx_fit_loo, bit for bit, then
 *   n_eff         = r_eff / sum w_i^2 over the cell's normalised PSIS weights w (r_eff = 1 where none is given);
 *   mcse_elpd_loo = sqrt(v / r_eff), v the variance (ddof 1) of log1p(c z_j) over the scores z_j = Phi^-1((j - 3/8) / 1000.25),
 *                   j = 1 .. 1000, with 1 + c z_j > 0, c = sqrt(sum w_i^2 expm1(log_lik_i - elpd_loo)^2), elpd_loo taken within the
 *                   range of the cell's log_lik (a constant column: c = 0, mcse_elpd_loo = 0).
 * A cell excluded by the model has uniform weights: n_eff = N r_eff (khat stays NaN). A cell that is NaN in ppcx_fit_loo is NaN in
 * both. The same bits on every call, whatever other genes are requested.                                                       */
#define PPCX_LOO_MCSE_FIELDS 6  /* elpd_loo, p_loo, looic, khat, mcse_elpd_loo, n_eff */
PPCX_API int ppcx_fit_loo_mcse(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double* out);
/* ppcx_fit_loo with a second attempt at the cells whose khat exceeds k_threshold: importance-weighted moment matching (Paananen,
 * Piironen, Buerkner, Vehtari 2021; loo::loo_moment_match), applied to the coordinates of the cell's own gene only -- intercept,
 * slopes of a checked gene, sigma_raw -- because given the hyper-parameters the posterior factorises over the genes: the affine
 * transform changes the log posterior by the gene's own likelihood and prior terms, so neither the full log density nor lp__ is
 * needed (a ppcx_fit_from_draws fit is served). A deliberate deviation from loo, which transforms every coordinate; restated from
 * the paper, not run against R. Per cell above the threshold, at most max_iters times: the draws of the gene are shifted to their
 * weighted mean, or, if that does not lower khat, shifted and scaled to their weighted mean and variance; a step is kept only if
 * the cell's PSIS khat on the new ratios is strictly lower. No covariance step (ppcx_fit_loo_moment_match_cov below adds it as a
 * third candidate), no split transformation: a matched khat is necessary, not sufficient (ppcx_fit_loo_moment_match_split below
 * adds the split transformation), and no mcse / n_eff is given for a matched cell.
 * Fits, genes, r_eff, limits and refusals as ppcx_fit_loo (an ADVI fit: PPCX_ERR_ARG, moment matching under the weights of
 * loo_approximate_posterior is ppcx_fit_loo_moment_match_approx); also PPCX_ERR_ARG for a k_threshold that is not finite or max_iters < 0.
 * out [n_genes][S][PPCX_LOO_MM_FIELDS(C)]: elpd_loo, p_loo (lpd of the original draws - elpd_loo), looic, khat (the final one),
 * khat_before (plain PSIS's), iterations (accepted steps), then scale[C + 1] and shift[C + 1] of the gene's coordinates in the
 * order intercept, slopes, sigma_raw: the matched draws are scale * draw + shift (a row the gene does not have: 1 and 0). A cell
 * that is excluded, NaN, at or below the threshold, run with max_iters = 0, or on which no step was accepted holds
 * ppcx_fit_loo's four fields bit for bit, khat_before = khat, iterations 0, scale 1, shift 0. The same bits on every call,
 * whatever other genes are requested.                                                                                          */
#define PPCX_LOO_MM_FIELDS(C) (6 + 2 * ((C) + 1))
PPCX_API int ppcx_fit_loo_moment_match(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                                       int max_iters, double* out);
/* ppcx_fit_loo_moment_match with the split transformation of Paananen et al. (2021, section 4; loo:::loo_moment_match_split, the
 * default of loo::loo_moment_match) on the cells it has matched (iterations > 0). The matched draws are no longer a sample of a
 * known density, so the matched estimate is biased; the split estimator transforms only the first h = n / 2 draws in the fit's
 * order (whole leading chains, as loo takes them), keeps the others, and weights all of them against the two-component mixture
 * they come from: draw i at its proposal point x_i (scale * draw_i + shift for i < h, draw_i from h on) has the log ratio
 * q(x_i) - log_lik(x_i) - logaddexp(q(x_i), q(T^-1 x_i) - sum log scale), q the gene's local log density; the terms of the log
 * posterior outside the gene are the same in both components and cancel, so a ppcx_fit_from_draws fit is served. PSIS runs on
 * these ratios as on a candidate of the matching; elpd_loo, p_loo (lpd of the original draws - elpd_loo) and looic are taken
 * under its weights. Restated from the paper and the published package; not run against R.
 * Fits, genes, r_eff, k_threshold, max_iters, limits and refusals as ppcx_fit_loo_moment_match (an ADVI fit: PPCX_ERR_ARG).
 * out [n_genes][S][PPCX_LOO_MM_SPLIT_FIELDS(C)]: ppcx_fit_loo_moment_match's record with elpd_loo, p_loo and looic the split
 * ones -- khat stays the matching's final one, as loo reports it, and khat_before, iterations, scale and shift are that entry's
 * bits -- then elpd_loo_matched (that entry's elpd_loo) and khat_split (the k-hat of the split ratios: a diagnostic, not a gate;
 * NaN for a cell with iterations = 0). A cell with iterations = 0 holds ppcx_fit_loo_moment_match's record bit for bit. A cell
 * none of whose split ratios is finite: elpd_loo, p_loo, looic and khat_split are NaN. No covariance step (that is
 * ppcx_fit_loo_moment_match_cov, which takes the split as an argument), no mcse / n_eff of a matched cell. The same bits on every
 * call, for any gene subset.                                                                                                   */
#define PPCX_LOO_MM_SPLIT_FIELDS(C) (PPCX_LOO_MM_FIELDS(C) + 2)
PPCX_API int ppcx_fit_loo_moment_match_split(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                                             int max_iters, double* out);
/* ppcx_fit_loo_moment_match with the covariance step as a third candidate (ppcx_loo_mm_cov.h; loo's shift_and_cov restated for
 * one gene; restated from the paper and the published package; not run against R). A gene's coordinates are correlated by
 * construction, and an outlying cell can move the posterior along a direction that no per-coordinate scale follows. The state
 * is an affine map (transform, shift) of the gene's coordinates, initially the identity; candidates 1 and 2 are the shift and
 * the shift with a per-coordinate scale on that state; candidate 3, tried when 1 is refused and 2 is refused or invalid, maps
 * the draws' mean and covariance over the gene's d coordinates onto their weighted mean and weighted covariance (the unbiased
 * form of stats::cov.wt) through the Cholesky factors of the two matrices. It is invalid, and so refused, when n <= d, when
 * 1 - sum w^2 is not positive, or when a pivot of either factor is not finite or <= 0. Gates, tail length, tie rule and r_eff as
 * ppcx_fit_loo_moment_match. split != 0: the split transformation of ppcx_fit_loo_moment_match_split on the matched cells with
 * the map, the identity and the map's inverse (carried along the accepted steps on the device) as its three states.
 * Fits, genes, r_eff, limits and refusals as ppcx_fit_loo_moment_match (an ADVI fit: PPCX_ERR_ARG; a ppcx_fit_from_draws fit is
 * served).
 * out [n_genes][S][PPCX_LOO_MM_COV_FIELDS(C)]: elpd_loo, p_loo, looic, khat (the matching's final one), khat_before, iterations
 * (accepted steps), cov_iterations (those of the third kind), elpd_loo_matched (the unsplit estimate; elpd_loo itself without
 * split), khat_split (NaN without split or with iterations = 0), transform [C + 1][C + 1] row-major and shift [C + 1] in the
 * order intercept, slopes, sigma_raw: the matched draws are transform * draw + shift (a row or column the gene does not have
 * is the identity's, its shift 0). A cell with iterations = 0 holds ppcx_fit_loo's four fields bit for bit, the identity and
 * zeros. The exact predictive under these weights is ppcx_fit_loo_predict_exact_moment_match_cov. Still left out: mcse / n_eff
 * of a matched cell, the covariance step for ADVI fits. The same bits on every call, for any gene subset.                                              */
#define PPCX_LOO_MM_COV_FIELDS(C) (9 + ((C) + 1) * ((C) + 1) + ((C) + 1))
PPCX_API int ppcx_fit_loo_moment_match_cov(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                                           int max_iters, int split, double* out);
/* The relative efficiency of the importance ratios per observed cell of a NUTS fit: what rstan::loo(fit) passes to loo::loo as
 * r_eff, loo::relative_eff(exp(log_lik), chain_id), so that ppcx_fit_loo / ppcx_fit_loo_predict with it report what rstan::loo(fit)
 * does without the log-likelihood matrix ever leaving the device. Fits, genes and refusals as ppcx_fit_loo; more than 128 chains:
 * PPCX_ERR_LIMIT (ppcx_fit_summary's bound). Synchronous on the model's stream; the same bits on every call, for any gene subset.
 *   out [n_genes][S]: ESS / N of v = exp(log_lik - max log_lik) over the split chains (each chain's first and last
 *   floor(n_keep / 2) draws; N values in 2 chains sequences), ESS the Geyer estimator of ppcx_fit_summary on v itself (no rank
 *   normalisation, no folding: posterior::ess_mean). The shift by the maximum does not change the ESS and keeps it defined where
 *   exp(log_lik) underflows. Values above 1 (antithetic chains) are kept. NaN: a NaN or +Inf log_lik, n_keep < 4, or all
 *   values equal; log_lik = -Inf is an ordinary value (v = 0). A cell excluded by the model gets a value like any other
 *   (ppcx_fit_loo does not use it). The caller replaces NaN (by 1, the default tail) before handing the array to ppcx_fit_loo,
 *   which refuses a non-finite r_eff.                                                                                          */
PPCX_API int ppcx_fit_relative_eff(ppcx_fit* f, int n_genes, const int32_t* genes, double* out);
/* The leave-one-out predictive interval and LOO-PIT per observed cell of a NUTS fit, from that ONE fit: for cell (g, s) the
 * distribution of its count under the posterior that has not seen the cell (what loo::E_loo(yrep, psis, type = "quantile" /
 * "mean") and bayesplot's ppc_loo_intervals / ppc_loo_pit give; ppcseq's question -- is the observed count inside the interval? --
 * without the second fit). Fits, genes, r_eff and refusals as ppcx_fit_loo; besides PPCX_ERR_ARG unless 0 <= p_lo < p_hi <= 1
 * and truncation_compensation is finite and > 0. Synchronous on the model's stream.
 *   out [n_genes][S][PPCX_LOO_PREDICT_FIELDS]: mean, lower, upper, pit_lt, pit_le, khat.
 *   The predictive count of kept draw i (all chains, the fit's order) is neg_binomial_2_log_rng(exposure_s + X_s alpha_g(i),
 *   truncation_compensation exp(-sigma_raw_g(i))) on the Philox address (seed, g S + s, i): for g < K the integers of
 *   ppcx_fit_ppc's counts_rng with n_gen = 0, resample = 0. Draw i carries the PSIS weight w_i of ppcx_fit_loo's cell (the tail
 *   smoothed in the order of a stable sort of the ratios: tied draws take the tail's positions in draw order); the compensation
 *   scales the predictive draw only, never the likelihood behind the weights. With F(v) = sum w_i 1[x_i <= v]:
 *   mean = sum w_i x_i; pit_lt = sum w_i 1[x_i < y], pit_le = F(y) (the two ends of the randomised LOO-PIT of the observed count
 *   y); lower, upper = Q(p_lo), Q(p_hi), loo's weighted quantile: v* the smallest drawn value with F(v*) >= p, Q = v* if no drawn
 *   value is below it, else Q = v- + (v* - v-) (p - F(v-)) / (F(v*) - F(v-)) with v- the largest drawn value below v*;
 *   khat as ppcx_fit_loo (above 0.7 the weights are not to be trusted).
 *   A cell excluded by the model at the time of the call is already held out: uniform weights, khat = NaN, mean, lower and upper
 *   equal ppcx_fit_ppc's mean, .lower and .upper (type-7 quantiles) bit for bit at the same seed, probabilities and compensation
 *   (g < K). A NaN log_lik, one of -Inf, or an invalid predictive draw: the cell is NaN. Neither the log-likelihood nor the
 *   counts matrix is materialised; the same bits on every call, for any gene subset. Tail limit as ppcx_fit_loo.              */
#define PPCX_LOO_PREDICT_FIELDS 6   /* mean, lower, upper, pit_lt, pit_le, khat */
PPCX_API int ppcx_fit_loo_predict(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double truncation_compensation,
                                  double p_lo, double p_hi, unsigned long long seed, double* out);
/* PSIS-LOO per observed cell of an ADVI fit: what loo::loo_approximate_posterior(log_lik, log_p, log_g) reports per observation
 * (Magnusson, Andersen, Jonasson, Vehtari 2019; restated from the published package, not run against R). The draws come from the
 * approximation g, so the log ratio of draw i for a cell is (log_p_i - log_g_i) - log_lik_i -- the first term is the array behind
 * ppcx_fit_get_log_ratios / ppcx_fit_psis, made on first use -- and PSIS runs on it with r_eff = 1 (the draws are independent).
 * Genes, cells, limits and layout as ppcx_fit_loo: out [n_genes][S][PPCX_LOO_FIELDS], elpd_loo = logsumexp(lw + log_lik) -
 * logsumexp(lw), p_loo = lpd - elpd_loo with lpd = logsumexp(log_lik) - log N unweighted, looic, khat. Tied ratios take the tail's
 * positions in draw order. A NaN log_lik or log ratio, or a ratio of +Inf: the cell is NaN; a ratio of -Inf (a draw whose log_p is
 * not finite) takes no part. A cell excluded by the model is already held out of p, but the draws are still g's: its ratios are
 * log_p - log_g alone, elpd_loo the same formula, p_loo = 0 and khat the overall k-hat of ppcx_fit_psis (column -1).
 * A NUTS fit, or one made by ppcx_fit_from_draws: PPCX_ERR_ARG (theirs is ppcx_fit_loo). The same bits on every call, for any gene
 * subset. The Monte-Carlo standard error and n_eff of ppcx_fit_loo_mcse are not available for these weights.                   */
PPCX_API int ppcx_fit_loo_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double* out);
/* ppcx_fit_loo_predict for an ADVI fit: the same predictive counts, quantiles, mean and LOO-PIT under the normalised weights of
 * ppcx_fit_loo_approx. A cell excluded by the model is weighted too (by log_p - log_g; it has no uniform path, and its khat is
 * the overall k-hat). out [n_genes][S][PPCX_LOO_PREDICT_FIELDS]; fits and refusals as ppcx_fit_loo_approx, probabilities and
 * truncation compensation as ppcx_fit_loo_predict.                                                                              */
PPCX_API int ppcx_fit_loo_predict_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation, double p_lo,
                                         double p_hi, unsigned long long seed, double* out);
/* The exact posterior-predictive tail probabilities and interval per cell of the checked genes: the Rao-Blackwellised form of the
 * model's `generated quantities`. Given kept draw i the count of cell (g, s) is neg_binomial_2_log(eta_i, phi_i), eta_i =
 * exposure_s + X_s alpha_g(i), phi_i = truncation_compensation exp(-sigma_raw_g(i)) as in ppcx_fit_ppc, so the posterior predictive
 * cdf of the cell is the plain average over the kept draws of negative-binomial cdfs (regularised incomplete beta functions,
 * evaluated on the device). Nothing is sampled: what remains is the Monte-Carlo error of the posterior draws themselves.
 * NUTS fits, ADVI fits and ppcx_fit_from_draws fits alike. genes: n_genes ids of checked genes (0 .. K - 1), or NULL with
 * n_genes = K for all of them. PPCX_ERR_ARG unless 0 < p_lo < p_hi < 1, truncation_compensation is finite and > 0 and every gene is
 * a checked one. Synchronous on the model's stream; the same bits on every call, for any gene subset.
 *   out [n_genes][S][PPCX_PPC_EXACT_FIELDS]:
 *   mean = mean_i e^{eta_i};  sd = sqrt(mean_i(mu_i + mu_i^2 / phi_i) + var_i(mu_i)) (ddof 0);
 *   p_le = P(X <= y), p_ge = P(X >= y) of the observed count y under the predictive distribution;
 *   lower, upper = the smallest integers k with F(k) >= p_lo, p_hi, F the predictive cdf: the inverse-cdf quantiles of the
 *   distribution. ppcx_fit_ppc reports type-7 SAMPLE quantiles, which interpolate between integers; the two agree in the limit of
 *   draws;  y;  excluded (0 / 1: reported only -- the predictive does not depend on whether the cell is in the likelihood);
 *   outside = (y < lower) | (y > upper) as 0 / 1.
 *   A draw with invalid parameters (a non-finite eta_i or e^{eta_i}, phi_i not finite and > 0) makes every statistic of the cell
 *   NaN (y and excluded are still reported).                                                                                    */
#define PPCX_PPC_EXACT_FIELDS 9     /* mean, sd, p_le, p_ge, lower, upper, y, excluded, outside */
PPCX_API int ppcx_fit_ppc_exact(ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation, double p_lo,
                                double p_hi, double* out);
/* The exact leave-one-out predictive tail probabilities and interval per cell of the checked genes of a NUTS fit: the fourth
 * corner beside ppcx_fit_ppc (sampled, posterior), ppcx_fit_ppc_exact (exact, posterior) and ppcx_fit_loo_predict (sampled,
 * leave-one-out). Given kept draw i the count of the cell is neg_binomial_2_log(eta_i, phi_i) as in ppcx_fit_ppc_exact, and draw i
 * carries the PSIS weight w_i of ppcx_fit_loo_predict's cell (the same ratios, tail, tie rule and normalisation; the truncation
 * compensation scales the predictive distribution only, never the likelihood behind the weights), so the leave-one-out
 * predictive cdf of the cell is the weighted average of negative-binomial cdfs. Nothing is sampled: a tail probability that
 * PSIS rests on a few heavy draws is not decided by as many sampled integers. In R: loo::E_loo on the draws' exact cdfs; no
 * function of loo or bayesplot does it. Restated from the published definitions, not run against R.
 * NUTS fits only (an ADVI fit: ppcx_fit_loo_predict_exact_approx; a ppcx_fit_from_draws fit holds the draws of a NUTS fit and
 * is taken as one). genes: n_genes ids of checked genes (0 .. K - 1); r_eff NULL (all 1) or [n_genes][S] as ppcx_fit_loo.
 * PPCX_ERR_ARG unless 0 < p_lo < p_hi < 1, truncation_compensation is finite and > 0, every gene is a checked one and every
 * r_eff is finite and > 0; tail limit as ppcx_fit_loo. Synchronous on the model's stream; the same bits on every call, for any
 * gene subset.
 *   out [n_genes][S][PPCX_LOO_EXACT_FIELDS]:
 *   mean = sum w_i mu_i;  sd = sqrt(sum w_i (mu_i + mu_i^2 / phi_i) + sum w_i (mu_i - mean)^2);
 *   p_le = sum w_i P_i(X <= y), p_ge = sum w_i P_i(X >= y): the two ends of the randomised LOO-PIT of the observed count y are
 *   1 - p_ge and p_le;
 *   lower, upper = the smallest integers k with F(k) >= p_lo, p_hi, F the weighted cdf, by ppcx_fit_ppc_exact's search;
 *   y;  excluded (0 / 1);  outside = (y < lower) | (y > upper) as 0 / 1;
 *   khat: ppcx_fit_loo_predict's khat of the cell, bit for bit (above 0.7 the weights are not to be trusted).
 *   A cell excluded by the model at the time of the call is already held out: uniform weights, its first nine fields are
 *   ppcx_fit_ppc_exact's bit for bit, khat = NaN. A draw with invalid parameters, a NaN log_lik or one of -Inf (a ratio of +Inf)
 *   in a cell that is not excluded: every statistic of the cell is NaN (y and excluded are still reported).                   */
#define PPCX_LOO_EXACT_FIELDS 10    /* mean, sd, p_le, p_ge, lower, upper, y, excluded, outside, khat */
PPCX_API int ppcx_fit_loo_predict_exact(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                        double truncation_compensation, double p_lo, double p_hi, double* out);
/* ppcx_fit_loo_predict_exact for an ADVI fit: the same fields under the normalised weights of ppcx_fit_loo_approx (ratios
 * (log_p - log_g) - log_lik on the cached log_p - log_g, r_eff = 1). A cell excluded by the model is weighted too (by
 * log_p - log_g; it has no uniform path, and its khat is the overall k-hat). A NUTS fit, or one made by ppcx_fit_from_draws:
 * PPCX_ERR_ARG (theirs is ppcx_fit_loo_predict_exact). Genes, probabilities and truncation compensation as above.             */
PPCX_API int ppcx_fit_loo_predict_exact_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation,
                                               double p_lo, double p_hi, double* out);
/* ppcx_fit_loo_predict_exact with a second attempt at the cells whose khat exceeds k_threshold: the cells a posterior-predictive
 * check exists to find are outliers, and an outlier is the cell whose plain PSIS weights are not to be trusted. Such a cell is
 * matched as ppcx_fit_loo_moment_match matches it (the same kernels, so khat, khat_before, iterations, scale and shift are that
 * entry's bits), and its predictive is importance sampling with the matched draws t_i = scale * draw_i + shift as the proposal:
 * the weights w_i are the normalised PSIS weights of the ratios q(t_i) - q(draw_i) - log_lik(t_i) (q the gene's local log
 * density; the constant Jacobian cancels), and eta_i, phi_i of the negative binomials are evaluated at t_i. Nothing is sampled.
 * Genes (checked ones), r_eff, probabilities, truncation compensation, limits and refusals as ppcx_fit_loo_predict_exact;
 * k_threshold and max_iters as ppcx_fit_loo_moment_match (PPCX_ERR_ARG for a k_threshold that is not finite or max_iters < 0).
 * An ADVI fit: PPCX_ERR_ARG (theirs is ppcx_fit_loo_predict_exact_moment_match_approx); a ppcx_fit_from_draws fit is served. No covariance step, no split transformation: a matched khat
 * is necessary, not sufficient (ppcx_fit_loo_predict_exact_moment_match_split below adds the split,
 * ppcx_fit_loo_predict_exact_moment_match_cov the covariance step). Synchronous on the model's stream; the same bits on every call, for any gene subset.
 *   out [n_genes][S][PPCX_LOO_MM_EXACT_FIELDS(C)]: the ten fields of ppcx_fit_loo_predict_exact with khat the final one, then
 *   khat_before (plain PSIS's), iterations (accepted steps), scale[C + 1] and shift[C + 1] as ppcx_fit_loo_moment_match.
 *   A cell with iterations = 0 (excluded, NaN, at or below the threshold, max_iters = 0, or no step accepted) holds
 *   ppcx_fit_loo_predict_exact's ten fields bit for bit (an excluded cell: ppcx_fit_ppc_exact's nine, khat = NaN). A matched
 *   draw with invalid parameters makes every statistic of the cell NaN, khat included (y, excluded and the record of the
 *   matching are still reported).                                                                                              */
#define PPCX_LOO_MM_EXACT_FIELDS(C) (12 + 2 * ((C) + 1))
PPCX_API int ppcx_fit_loo_predict_exact_moment_match(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                                     double k_threshold, int max_iters, double truncation_compensation,
                                                     double p_lo, double p_hi, double* out);
/* ppcx_fit_loo_predict_exact_moment_match with the split transformation (ppcx_fit_loo_moment_match_split) on the cells it has
 * matched: the weights are the normalised PSIS weights of the split ratios, and eta_i, phi_i of the negative binomials are
 * evaluated at the proposal points x_i -- scale * draw_i + shift for the first h = n / 2 draws in the fit's order, draw_i from h
 * on. Arguments, limits and refusals as ppcx_fit_loo_predict_exact_moment_match.
 *   out [n_genes][S][PPCX_LOO_MM_EXACT_SPLIT_FIELDS(C)]: that entry's record with the first nine fields under the split weights and
 *   khat the matching's final one, then khat_split (NaN for a cell with iterations = 0, which holds that entry's record bit for
 *   bit). A proposal point with invalid parameters, or no finite split ratio: every statistic of the cell is NaN, khat and
 *   khat_split included. The same bits on every call, for any gene subset.                                                     */
#define PPCX_LOO_MM_EXACT_SPLIT_FIELDS(C) (PPCX_LOO_MM_EXACT_FIELDS(C) + 1)
PPCX_API int ppcx_fit_loo_predict_exact_moment_match_split(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                                           double k_threshold, int max_iters, double truncation_compensation,
                                                           double p_lo, double p_hi, double* out);
/* ppcx_fit_loo_predict_exact with the cells above k_threshold matched first as ppcx_fit_loo_moment_match_cov matches them (the same
 * kernels, so khat, khat_before, iterations, cov_iterations, transform and shift are that entry's bits), then the predictive
 * under those weights at the affinely matched draws transform * draw_i + shift (ppcx_loo_mm_cov_exact.h). split != 0: the
 * weights are the normalised PSIS weights of the split ratios of ppcx_fit_loo_moment_match_cov(split), formed on the transform,
 * the identity and the inverse accumulated along the accepted steps; eta_i, phi_i are evaluated at the proposal points --
 * transform * draw_i + shift for the first h = n / 2 draws in the fit's order, draw_i from h on. Nothing is sampled.
 * Arguments, limits and refusals as ppcx_fit_loo_predict_exact_moment_match: checked genes only, an ADVI fit is PPCX_ERR_ARG, a
 * ppcx_fit_from_draws fit and pooled chains are served.
 *   out [n_genes][S][PPCX_LOO_MM_COV_EXACT_FIELDS(C)]: the ten fields of ppcx_fit_loo_predict_exact with khat the matching's final
 *   one, then khat_before, iterations, cov_iterations, khat_split (NaN without split or with iterations = 0), transform
 *   [C + 1][C + 1] row-major and shift [C + 1]. A cell with iterations = 0 holds ppcx_fit_loo_predict_exact's ten fields bit for
 *   bit. A proposal point with invalid parameters, or no finite ratio: every statistic of the cell is NaN, khat and khat_split
 *   included. Left out: mcse / n_eff of a matched cell, the covariance step for ADVI fits. The same bits on every call, for any gene subset.          */
#define PPCX_LOO_MM_COV_EXACT_FIELDS(C) (14 + ((C) + 1) * ((C) + 1) + ((C) + 1))
PPCX_API int ppcx_fit_loo_predict_exact_moment_match_cov(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                                         double k_threshold, int max_iters, int split,
                                                         double truncation_compensation, double p_lo, double p_hi, double* out);
/* ppcx_fit_loo_approx with a second attempt at the cells whose khat exceeds k_threshold: the gene-local moment matching of
 * ppcx_fit_loo_moment_match for draws that come from the approximation g of an ADVI fit (ppcx_loo_mm_ap.h). An affine map of the
 * gene's own coordinates is an implicit change of proposal with a constant Jacobian, and given the hyper-parameters the posterior
 * factorises over the genes, so the log ratio of a candidate state is (log_p_i - log_g_i) + q(t_i) - q(draw_i) - log_lik(t_i), q
 * the gene's local log density: ppcx_fit_loo_moment_match's ratio plus the cached array of ppcx_fit_psis. Neither log_g at a new
 * point nor the approximation's (mu, omega) is needed. loo::loo_moment_match has no approximate-posterior form: a deliberate
 * deviation from loo, restated from Paananen et al. (2021) and Magnusson et al. (2019), not run against R. Candidates (shift;
 * shift and scale), gate (a strictly lower khat), tail and tie rule as ppcx_fit_loo_moment_match; r_eff = 1.
 * Fits, genes, limits and refusals as ppcx_fit_loo_approx (a NUTS fit, or one made by ppcx_fit_from_draws: PPCX_ERR_ARG); also
 * PPCX_ERR_ARG for a k_threshold that is not finite or max_iters < 0.
 * out [n_genes][S][PPCX_LOO_MM_FIELDS(C)], the layout of ppcx_fit_loo_moment_match. A cell that is excluded (its khat is the
 * overall k-hat), NaN, at or below the threshold, run with max_iters = 0, or on which no step was accepted holds
 * ppcx_fit_loo_approx's four fields bit for bit, khat_before = khat, iterations 0, scale 1, shift 0.
 * Left out: the split transformation (for a proposal g it needs log_g at inverse-mapped points), the covariance step, mcse /
 * n_eff, passes over several ranks. A matched khat below the threshold is therefore necessary, not sufficient; and the matching
 * moves one gene's coordinates only -- where the overall k-hat of log_p - log_g is itself above the threshold the mismatch sits in
 * the hyper-parameters as well, which no map of a gene's coordinates repairs: a cell's khat below the threshold does not speak
 * for that part (it is an estimate of the cell's own ratios and can lie below the overall one). The same bits on every call, for
 * any gene subset.                                                                                                              */
PPCX_API int ppcx_fit_loo_moment_match_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double k_threshold, int max_iters,
                                              double* out);
/* ppcx_fit_loo_predict_exact_approx with the cells above k_threshold matched first as ppcx_fit_loo_moment_match_approx matches them
 * (the same kernels, so khat, khat_before, iterations, scale and shift are that entry's bits), then the predictive under those
 * weights with eta_i, phi_i of the negative binomials evaluated at the matched draws, as ppcx_fit_loo_predict_exact_moment_match
 * does for a NUTS fit. Genes (checked ones), probabilities and truncation compensation as ppcx_fit_loo_predict_exact_approx;
 * k_threshold, max_iters, refusals and what is left out as ppcx_fit_loo_moment_match_approx.
 *   out [n_genes][S][PPCX_LOO_MM_EXACT_FIELDS(C)], the layout of ppcx_fit_loo_predict_exact_moment_match. A cell with
 *   iterations = 0 holds ppcx_fit_loo_predict_exact_approx's ten fields bit for bit. The same bits on every call, for any gene
 *   subset.                                                                                                                    */
PPCX_API int ppcx_fit_loo_predict_exact_moment_match_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double k_threshold,
                                                            int max_iters, double truncation_compensation, double p_lo, double p_hi,
                                                            double* out);
/* lp: [chains][n_keep]; the rest [chains][iter] (warmup included); any pointer may be NULL */
PPCX_API int ppcx_fit_get_diagnostics(ppcx_fit* f, double* lp, double* stepsize, int32_t* treedepth,
                             int32_t* n_leapfrog, int32_t* divergent, double* accept);
/* [chains][D]: the diagonal of the inverse metric every chain ended its warm-up with, in the order of the unconstrained vector
 * (what rstan::get_adaptation_info(fit) prints as "Diagonal elements of inverse mass matrix"; the adapted step sizes are the
 * last column of ppcx_fit_get_diagnostics' stepsize). NUTS fits only.                                                        */
PPCX_API int ppcx_fit_get_inv_metric(ppcx_fit* f, double* inv_metric);
/* wall seconds of the sampling loop, gradient evaluations summed over chains, and the mean duration
 * (ms) / count of the HIP-event-timed log-likelihood-kernel launches with the chain-launches they covered    */
PPCX_API int ppcx_fit_get_timing(ppcx_fit* f, double* seconds, long long* grad_evals, double* gene_kernel_ms_mean,
                        long long* gene_kernel_samples, double* gene_kernel_chain_launches_mean);

/* mean HIP-event durations (ms) of the three kernels of a leapfrog over the timed launches, and the number of
 * (loglik, close, update) launch triples the run issued                                                   */
PPCX_API int ppcx_fit_get_kernel_times(ppcx_fit* f, double* loglik_ms, double* close_ms, double* update_ms,
                              long long* launch_triples);

/* generated quantities + credible intervals (.stan:259-266; R/utilities.R:685-703 full analysis,
 * :733-784 approximated analysis when resample != 0 and n_gen = how_many_posterior_draws).
 * ci: [K][S][4] = mean, sd, lower, upper.  counts_rng: NULL or [n_gen][K][S] int32.
 * n_gen = 0 means one predictive draw per kept posterior draw.                                      */
PPCX_API int ppcx_fit_ppc(ppcx_fit* f, double truncation_compensation, double p_lo, double p_hi,
                 unsigned long long seed, int n_gen, int resample, double* ci, int32_t* counts_rng);
/* duration (ms, HIP events) of the posterior-predictive kernel of the last ppcx_fit_ppc call and the negative-binomial
 * draws it generated (n_gen x K x S)                                                                                   */
PPCX_API int ppcx_fit_get_ppc_timing(ppcx_fit* f, double* kernel_ms, long long* nb_draws);
PPCX_API void ppcx_fit_free(ppcx_fit* f);

/* R .C() convention (all pointers, void return; character vectors arrive as char**): one do_inference() pass end to end --
 * what R/utilities.R:1482-1531 obtains from vb_iterative()/sampling(), summary(fit, "counts_rng"), extract() and
 * summary(fit, "alpha_sub_1").
 *   dims[33] = {PPCX_VERSION the caller was written for (anything else: status PPCX_ERR_ARG, nothing else is read),
 *               device, G, S, C, K, n_excl, chains, iter, warmup, n_gen, resample,
 *               approximate_posterior_inference (0 = NUTS, R/utilities.R:1497-1512; 1 = ADVI through the bounded
 *               vb_iterative retry, :1487-1494), save_generated_quantities (counts_rng is filled, :796),
 *               vb_output_samples, vb_iter (0 = 50000),
 *               n_devices (0: the one `device` above), devices[16] (the first n_devices are read)}
 *             With n_devices > 1 a NUTS pass deals its chains to those devices -- a host thread each, as rstan::sampling runs
 *             its chains on `cores` workers (R/utilities.R:1500-1501) -- and summarises the pooled chains on the first one;
 *             the result is that of one device running all the chains. A device may be named more than once.
 *   reals[6] = {lambda_mu_mu, truncation_compensation, p_lo, p_hi, seed, vb_tol_rel_obj (0 = 0.005, the value the
 *               reference hard-codes at :1492)}
 *   outputs  : ci [K*S*4] (mean, sd, .lower, .upper per checked cell), slope [K] (posterior mean of alpha_sub_1),
 *              counts_rng [n_draws*K*S] or NULL, status[1] (0 or a PPCX_ERR_* class), errbuf[0] (message, at most
 *              errlen[0] bytes including the terminator; may be NULL). No exception and no R condition crosses the ABI.   */
PPCX_API void ppcx_do_inference_C(const int* dims, const int* counts, const double* X, const double* exposure_rate,
                         const int* excl, const double* reals, double* ci, double* slope, int* counts_rng,
                         int* status, char** errbuf, const int* errlen);

/* --- ADVI = rstan::vb(model, output_samples, iter = 50000, tol_rel_obj = 0.005) through vb_iterative
 * (R/utilities.R:246-278, :1487-1494): mean-field Gaussian on the unconstrained scale, Stan defaults
 * grad_samples 1, elbo_samples 100, eval_elbo 100, adapt_iter 50. The result is a one-chain fit holding
 * output_samples draws of the approximation, so ppcx_fit_ppc / ppcx_fit_get_columns apply unchanged.          */
typedef struct {
  int output_samples, iter; double tol_rel_obj; int grad_samples, elbo_samples, eval_elbo, adapt_iter;
  unsigned long long seed; double init_radius;
} ppcx_advi_config;
PPCX_API void ppcx_advi_config_default(ppcx_advi_config* cfg);
PPCX_API int ppcx_fit_advi(ppcx_model* m, const ppcx_advi_config* cfg, ppcx_fit** out);
/* vb_iterative (R/utilities.R:246-278): retried with seed + attempt while ADVI fails to initialise or to find a step size */
PPCX_API int ppcx_fit_advi_iterative(ppcx_model* m, const ppcx_advi_config* cfg, int max_attempts, ppcx_fit** out);
PPCX_API int ppcx_fit_advi_info(const ppcx_fit* f, int* iterations, int* converged, double* elbo, double* eta);

/* --- gene shards = the reference's map_rect over gene shards (inst/stan/negBinomial_MPI.stan:226-240;
 * round-robin gene->shard assignment R/utilities.R:130-136; here contiguous gene ranges or the same round-robin deal,
 * ppcx_model_create_shard_strided). A shard model holds
 * genes [g0, g1) of a G_total-gene problem whose first K_total genes are the checked ones; the six
 * hyper-parameters are replicated and every leapfrog exchanges one vector of <= 76 partial sums (log density,
 * 6 hyper-gradient sums, kinetic energies, U-turn dot products).
 *   ppcx_fit_nuts_shards : all shards in this process on one device (testing, or splitting oversize problems)
 *   ppcx_fit_nuts_comm   : one shard per process / GPU, sums all-reduced with RCCL over xGMI              */
typedef struct ppcx_comm ppcx_comm;
PPCX_API int ppcx_model_create_shard(int device, int G_total, int S, int C, int K_total, int g0, int g1,
                            const int32_t* counts_shard, const double* X, const double* exposure_rate,
                            double lambda_mu_mu, int n_excl, const int32_t* excl_local, ppcx_model** out);
/* ... or every gene_stride-th gene from g0 on: genes g0, g0 + gene_stride, ..., n_genes of them (counts_shard holds their rows in
   that order). Shard r of N with g0 = r, gene_stride = N is the reference's round-robin deal (R/utilities.R:125-136): every shard
   gets its share of the K_total checked genes, which come first in the whole problem -- and with them an equal share of the work
   (a contiguous split gives the first shard every gene with a slope). Philox streams are addressed by the coordinate's index in
   the whole problem either way: a sharded run draws what the unsharded run draws. */
PPCX_API int ppcx_model_create_shard_strided(int device, int G_total, int S, int C, int K_total, int g0, int gene_stride, int n_genes,
                            const int32_t* counts_shard, const double* X, const double* exposure_rate,
                            double lambda_mu_mu, int n_excl, const int32_t* excl_local, ppcx_model** out);
PPCX_API int ppcx_fit_nuts_shards(ppcx_model** shards, int n_shards, const ppcx_nuts_config* cfg, ppcx_fit** fits);
PPCX_API int ppcx_comm_unique_id(char* out128);               /* rank 0 creates it, the host layer broadcasts it */
PPCX_API int ppcx_comm_create(int device, int nranks, int rank, const char* id128, ppcx_comm** out);
PPCX_API void ppcx_comm_destroy(ppcx_comm* c);
PPCX_API int ppcx_fit_nuts_comm(ppcx_model* shard, const ppcx_nuts_config* cfg, ppcx_comm* comm, ppcx_fit** out);

/* --- gene shards with a DIRECT exchange (the default between GPUs; exercised so far between processes that share one GPU and
 * between host threads -- no multi-GPU box was available to any round -- so the host layer, distributed.do_inference_shards, falls
 * back to ppcx_fit_nuts_comm on ALL ranks when its set-up fails on any): no collective library call per leapfrog. Every rank's
 * receive buffer (uncached device memory) is mapped into every rank -- hipIpc handles between processes -- and the chains'
 * state machines, which run inside the merged launch of a pipelined round beside the log-likelihood workgroups, store their
 * <= 76 partial sums into the peers' buffers over xGMI, then a sequence number, and wait for the peers' (rank-order sum:
 * identical bits, hence identical decisions, on every rank). A peer that leaves the fit or does not arrive within the timeout
 * fails the fit with PPCX_ERR_STALL on every rank. Needs a model that runs pipelined rounds (ppcx_model_get_rounds); the RCCL
 * path above serves the others.
 *   rank r: ppcx_xchg_create -> ppcx_xchg_handle (64 bytes) -> [host layer all-gathers the handles] -> ppcx_xchg_connect
 *           -> ppcx_fit_nuts_xchg (any number of fits, the same sequence on every rank) -> ppcx_xchg_destroy              */
typedef struct ppcx_xchg ppcx_xchg;
PPCX_API int ppcx_xchg_create(int device, int nranks, int rank, int max_chains, ppcx_xchg** out);
PPCX_API int ppcx_xchg_handle(ppcx_xchg* x, char* out64);
PPCX_API int ppcx_xchg_connect(ppcx_xchg* x, const char* handles /* nranks x 64 bytes, rank order */);
PPCX_API int ppcx_xchg_connect_local(ppcx_xchg** group, int n);   /* all ranks in this process (a host thread each) */
PPCX_API int ppcx_xchg_set_timeout(ppcx_xchg* x, double seconds); /* default 20 s */
PPCX_API void ppcx_xchg_destroy(ppcx_xchg* x);
PPCX_API int ppcx_fit_nuts_xchg(ppcx_model* shard, const ppcx_nuts_config* cfg, ppcx_xchg* x, ppcx_fit** out);
/* mean time (us) a chain's state machine waited for its peers per exchange, and the number of exchanges of the fit */
PPCX_API int ppcx_fit_get_xchg_timing(ppcx_fit* f, double* wait_us_per_exchange, long long* exchanges);

/* What the ranks of a gene-sharded run conclude at a poll from the max-reduced vector
 * [rounds, -rounds, chains done, -chains done, -(error status)] and their own status: PPCX_OK, the peer's / own error
 * class, or PPCX_ERR_STALL when the ranks disagree. Pure host logic, exported so that it can be tested without two GPUs. */
PPCX_API int ppcx_guard_decision(const double* reduced5, int local_status);

#ifdef __cplusplus
}
#endif
#endif
