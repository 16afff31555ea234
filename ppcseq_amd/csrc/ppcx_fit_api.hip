// ppcx_fit_api.hip -- what is read from a fit: its release, a fit over draws made elsewhere, draws, columns, summary, diagnostics
// and timings, the per-cell diagnostics (PSIS-LOO, LOO predictive, relative efficiency, exact posterior- and LOO-predictive tails) with
// their testing twins, and the posterior-predictive check.
#include <math.h>
#include <string.h>
#include "ppcx_host.h"
#include "ppcx_summary.h"
#include "ppcx_psis.h"
#include "ppcx_loo.h"

extern "C" void ppcx_fit_free(ppcx_fit* f) {
  if (!f) return;
  ppcx_model* m = f->m;
  (void)hipSetDevice(m->device);                 // the fit's buffers are freed on the current device
  delete f;
  if (--m->live_fits == 0 && m->destroy_requested) ppcx_model_destroy(m);
}

// A fit that holds draws produced elsewhere (other ranks' chains gathered by the host layer): ppcx_fit_ppc and
// ppcx_fit_get_columns then work on the pooled posterior, as rstan::summary does over merged chains (R/utilities.R:685-703).
extern "C" int ppcx_fit_from_draws(ppcx_model* m, int chains, int n_keep, const double* draws, ppcx_fit** out) {
  if (!m || !draws || !out || chains < 1 || n_keep < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  *out = nullptr;
  HIPCHK(hipSetDevice(m->device));
  ppcx_fit* f = new ppcx_fit();
  fit_attach(f, m); f->chains = chains; f->n_keep = n_keep; f->iter = n_keep;
  memset(&f->cfg, 0, sizeof f->cfg);
  const size_t n = (size_t)chains * n_keep * m->d.D;
  hipError_t e = f->d_draws.alloc(n);
  if (e == hipSuccess) e = hipMemcpy(f->d_draws.p, draws, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) { ppcx_fit_free(f); return fail(PPCX_ERR_HIP, hipGetErrorString(e)); }
  *out = f;
  return PPCX_OK;
}

extern "C" int ppcx_fit_info(const ppcx_fit* f, int* chains, int* n_keep, int* D, int* iter) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (chains) *chains = f->chains;
  if (n_keep) *n_keep = f->n_keep;
  if (D) *D = f->m->d.D;
  if (iter) *iter = f->iter;
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_draws(ppcx_fit* f, double* out) {
  if (!f || !out) return fail(PPCX_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(f->m->device));
  if (f->n_keep > 0) HIPCHK(hipMemcpy(out, f->d_draws.p, sizeof(double) * (size_t)f->chains * f->n_keep * f->m->d.D, hipMemcpyDeviceToHost));
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_columns(ppcx_fit* f, int n_cols, const int32_t* cols, double* out) {
  if (!f || !cols || !out || n_cols < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  const int D = f->m->d.D;
  for (int i = 0; i < n_cols; ++i) if (cols[i] < 0 || cols[i] >= D) return fail(PPCX_ERR_ARG, "column out of range");
  HIPCHK(hipSetDevice(f->m->device));
  const long rows = (long)f->chains * f->n_keep;
  if (rows == 0) return PPCX_OK;
  hipStream_t st = f->m->stream.s;
  DeviceBuffer<int> d_cols; DeviceBuffer<double> d_out;
  hipError_t e = d_cols.upload(cols, (size_t)n_cols, st);
  if (e == hipSuccess) e = d_out.alloc((size_t)rows * n_cols);
  if (e == hipSuccess) e = launch_gather_kernel(f->d_draws.p, rows, D, d_cols.p, n_cols, d_out.p, st);
  if (e == hipSuccess) e = d_out.download(out, (size_t)rows * n_cols, st);
  if ((e = finish(e, st)) != hipSuccess) return fail(PPCX_ERR_HIP, hipGetErrorString(e));
  return PPCX_OK;
}
// Fit summary (rstan::monitor): the columns go through column-major scratch in batches of at most kSummaryScratchBytes (never a
// second copy of all the draws), one workgroup per column (ppcx_summary.hip)
extern "C" int ppcx_fit_summary(ppcx_fit* f, int n_cols, const int32_t* cols, double* out) {
  if (!f || !cols || !out || n_cols < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  if (f->advi) return fail(PPCX_ERR_ARG, "an ADVI fit has independent draws: R-hat and ESS are not defined for it (rstan::vb reports neither)");
  const int D = f->m->d.D, M = f->chains, n = f->n_keep;
  for (int i = 0; i < n_cols; ++i) {
    if (cols[i] < -1 || cols[i] >= D) return fail(PPCX_ERR_ARG, "column out of range");
    if (cols[i] == -1 && !f->d_lp.p) return fail(PPCX_ERR_ARG, "this fit holds no lp__ (a fit over draws produced elsewhere)");
  }
  if (M < 1 || n < 1) return fail(PPCX_ERR_ARG, "fit holds no kept draws");
  if (M > kSummaryMaxChains) return fail(PPCX_ERR_LIMIT, "ppcx_fit_summary takes at most 128 chains");
  HIPCHK(hipSetDevice(f->m->device));
  const hipError_t e = summary_columns(f->d_draws.p, f->d_lp.p, M, n, D, n_cols, cols, out, kSummaryScratchBytes, f->m->stream.s);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, hipGetErrorString(e));
  return PPCX_OK;
}
// ---- PSIS-LOO per observed cell of a NUTS fit (rstan::loo / loo::loo on the cells' log-likelihood)
static size_t loo_scratch_bytes() {
#ifdef PPCX_TESTING
  if (g_test.loo_scratch_bytes > 0) return (size_t)g_test.loo_scratch_bytes;
#endif
  return kPsisScratchBytes;
}
// the fit, the genes, the cells' counts (an excluded cell as -(y + 1), kept in yenc) and the output as the record of these
// cells, whatever produced the fit's draws; sets the fit's device
static int loo_prepare_cells(ppcx_fit* f, int n_genes, const int32_t* genes, const void* out, std::vector<int>& yenc, FitCells& fc) {
  if (!genes || n_genes < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  if ((long)f->chains * f->n_keep < 1) return fail(PPCX_ERR_ARG, "fit holds no kept draws");
  const ppcx_model* m = f->m;
  const int G = m->d.G, S = m->d.S;
  for (int i = 0; i < n_genes; ++i) if (genes[i] < 0 || genes[i] >= G) return fail(PPCX_ERR_ARG, "gene out of range");
  yenc.resize((size_t)n_genes * S);
  for (int i = 0; i < n_genes; ++i)
    for (int s = 0; s < S; ++s) {
      const size_t c = (size_t)genes[i] * S + s;
      const int y = m->counts_host[c];
      yenc[(size_t)i * S + s] = m->excluded_host[c] ? -y - 1 : y;
    }
  HIPCHK(hipSetDevice(m->device));
  if (!out) return fail(PPCX_ERR_ARG, "bad arguments");
  fc.draws = f->d_draws.p; fc.n = (long)f->chains * f->n_keep; fc.chains = f->chains; fc.n_keep = f->n_keep;
  fc.d = m->d; fc.expo = m->d_expo.p; fc.X = m->d_X.p;
  fc.n_genes = n_genes; fc.genes = genes; fc.yenc = yenc.data();
  return PPCX_OK;
}
// ... of a NUTS fit
static int loo_prepare(ppcx_fit* f, int n_genes, const int32_t* genes, const void* out, std::vector<int>& yenc, FitCells& fc) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (f->advi) return fail(PPCX_ERR_ARG, "PSIS-LOO needs the draws of a NUTS fit (loo_approximate_posterior for ADVI fits is "
                                         "not available)");
  return loo_prepare_cells(f, n_genes, genes, out, yenc, fc);
}
extern "C" int ppcx_fit_get_log_lik(ppcx_fit* f, int n_genes, const int32_t* genes, double* out) {
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_prepare(f, n_genes, genes, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done("ppcx_fit_get_log_lik", loo_fit_log_lik(fc, out, loo_scratch_bytes(), f->m->stream.s));
}
// r_eff of `cells` cells of n draws (null: all 1): every value finite and > 0; *r_eff_min the smallest (the longest tail of the
// cells, for the selection buffer), whose tail has to fit that buffer. who: the entry point, null in the testing build
static int loo_reff_limits(const char* who, const double* r_eff, long cells, long n, double* r_eff_min) {
  double mn = 1.0;
  for (long i = 0; r_eff && i < cells; ++i) {
    if (!(isfinite(r_eff[i]) && r_eff[i] > 0.0)) return fail(PPCX_ERR_ARG, "r_eff must be finite and > 0");
    mn = i == 0 || r_eff[i] < mn ? r_eff[i] : mn;
  }
  if (psis_tail_len(n, mn) + 1 > kPsisMaxSel)
    return fail(PPCX_ERR_LIMIT, who ? std::string(who) + ": the tail exceeds 4095 draws" : std::string("too many draws"));
  *r_eff_min = mn;
  return PPCX_OK;
}
static int loo_fit_reff(const char* who, FitCells& fc, const double* r_eff) {
  fc.r_eff = r_eff;
  return loo_reff_limits(who, r_eff, (long)fc.n_genes * fc.d.S, fc.n, &fc.r_eff_min);
}
// ppcx_fit_loo (fields = kLooFields) and ppcx_fit_loo_mcse (kLooMcseFields): the same checks, limits and walk
static int fit_loo(const char* who, ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, int fields, double* out) {
  std::vector<int> yenc; FitCells fc;
  int rc = loo_prepare(f, n_genes, genes, out, yenc, fc);
  if (rc == PPCX_OK) rc = loo_fit_reff(who, fc, r_eff);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_fit_cells(fc, fields, out, loo_scratch_bytes(), f->m->stream.s));
}
extern "C" int ppcx_fit_loo(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double* out) {
  return fit_loo("ppcx_fit_loo", f, n_genes, genes, r_eff, kLooFields, out);
}
extern "C" int ppcx_fit_loo_mcse(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double* out) {
  return fit_loo("ppcx_fit_loo_mcse", f, n_genes, genes, r_eff, kLooMcseFields, out);
}
static int loo_exact_check(const ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation, double p_lo, double p_hi);
// ---- gene-local moment matching of the cells with a high k-hat (loo::loo_moment_match restated per gene; ppcx_loo_mm.h)
// The checks of the four moment-matching entries and the cells of the fit. probs: the predictive forms' truncation
// compensation, p_lo and p_hi, which add loo_exact_check (checked genes only); null: the elpd forms, which leave a NULL fit to
// loo_prepare.
static int loo_mm_prepare(const char* who, ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                          int max_iters, const double* probs, const void* out, std::vector<int>& yenc, FitCells& fc) {
  if (probs && !f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (f && f->advi)
    return fail(PPCX_ERR_ARG, std::string(who) + " needs the draws of a NUTS fit: moment matching under the weights of an ADVI fit "
                                                 "(loo_approximate_posterior) is ppcx_fit_loo_moment_match_approx and "
                                                 "ppcx_fit_loo_predict_exact_moment_match_approx, without the split transformation "
                                                 "and the covariance step");
  if (!isfinite(k_threshold)) return fail(PPCX_ERR_ARG, std::string(who) + ": k_threshold must be finite");
  if (max_iters < 0) return fail(PPCX_ERR_ARG, std::string(who) + ": max_iters must be >= 0");
  int rc = probs ? loo_exact_check(f, n_genes, genes, probs[0], probs[1], probs[2]) : PPCX_OK;
  if (rc == PPCX_OK) rc = probs ? loo_prepare_cells(f, n_genes, genes, out, yenc, fc) : loo_prepare(f, n_genes, genes, out, yenc, fc);
  if (rc == PPCX_OK) rc = loo_fit_reff(who, fc, r_eff);
  return rc;
}
// The elpd forms: the checks, the cells, then walk(fc, scratch_bytes, stream) -- the entry's driver over them
template <class Walk>
static int loo_mm_elpd_entry(const char* who, ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                             int max_iters, double* out, Walk walk) {
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_mm_prepare(who, f, n_genes, genes, r_eff, k_threshold, max_iters, nullptr, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, walk(fc, loo_scratch_bytes(), f->m->stream.s));
}
extern "C" int ppcx_fit_loo_moment_match(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                                         int max_iters, double* out) {
  return loo_mm_elpd_entry("ppcx_fit_loo_moment_match", f, n_genes, genes, r_eff, k_threshold, max_iters, out,
                           [&](const FitCells& fc, size_t bytes, hipStream_t st) { return loo_mm_fit_cells(fc, k_threshold, max_iters, out, bytes, st); });
}
// ... with the split transformation of the matched cells (ppcx_loo_mm_split.h): the matching's kernels, then the split
extern "C" int ppcx_fit_loo_moment_match_split(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                                               int max_iters, double* out) {
  return loo_mm_elpd_entry("ppcx_fit_loo_moment_match_split", f, n_genes, genes, r_eff, k_threshold, max_iters, out,
                           [&](const FitCells& fc, size_t bytes, hipStream_t st) {
    return loo_mm_split_fit_cells(fc, k_threshold, max_iters, false, 1.0, 0.0, 1.0, out, bytes, st);
  });
}
// ... with the covariance step as the third candidate (ppcx_loo_mm_cov.h); split != 0: the split transformation of the matched
// cells under the affine map, in the same kernel
extern "C" int ppcx_fit_loo_moment_match_cov(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double k_threshold,
                                             int max_iters, int split, double* out) {
  return loo_mm_elpd_entry("ppcx_fit_loo_moment_match_cov", f, n_genes, genes, r_eff, k_threshold, max_iters, out,
                           [&](const FitCells& fc, size_t bytes, hipStream_t st) {
    return loo_mm_cov_fit_cells(fc, k_threshold, max_iters, split != 0, out, bytes, st);
  });
}
// ---- the leave-one-out predictive interval and LOO-PIT of the same cells (loo::E_loo / bayesplot::ppc_loo_intervals, ppc_loo_pit)
static int loo_predict_check_probs(double p_lo, double p_hi) {
  if (!(p_lo >= 0.0 && p_lo < p_hi && p_hi <= 1.0)) return fail(PPCX_ERR_ARG, "need 0 <= p_lo < p_hi <= 1");
  return PPCX_OK;
}
extern "C" int ppcx_fit_loo_predict(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff, double truncation_compensation,
                                    double p_lo, double p_hi, unsigned long long seed, double* out) {
  const char* who = "ppcx_fit_loo_predict";
  std::vector<int> yenc; FitCells fc;
  int rc = loo_prepare(f, n_genes, genes, out, yenc, fc);
  if (rc == PPCX_OK) rc = loo_predict_check_probs(p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  if (!(isfinite(truncation_compensation) && truncation_compensation > 0.0))
    return fail(PPCX_ERR_ARG, "truncation_compensation must be finite and > 0");
  if ((rc = loo_fit_reff(who, fc, r_eff)) != PPCX_OK) return rc;
  return hip_done(who, loo_predict_fit_cells(fc, truncation_compensation, p_lo, p_hi, seed32(seed), out, loo_scratch_bytes(),
                                             f->m->stream.s));
}
// ---- the same two for an ADVI fit (loo::loo_approximate_posterior; ppcx_loo_ap.h): the draws come from the approximation, the
// ratios carry log_p - log_g, cached by the first call (psis_ratios)
static int loo_approx_prepare(const char* who, ppcx_fit* f, int n_genes, const int32_t* genes, const void* out, std::vector<int>& yenc,
                              FitCells& fc) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (!f->advi || !f->d_mu.p)
    return fail(PPCX_ERR_ARG, std::string(who) + " needs an ADVI fit: a NUTS fit, or one over draws produced elsewhere, holds no "
                                                 "approximation to correct for (PSIS-LOO of a NUTS fit is ppcx_fit_loo)");
  const int rc = loo_prepare_cells(f, n_genes, genes, out, yenc, fc);
  return rc == PPCX_OK ? loo_fit_reff(who, fc, nullptr) : rc;
}
// the last step before the walk: log_p - log_g of the draws on the device
static int loo_approx_ratios(ppcx_fit* f, FitCells& fc) {
  const int rc = psis_ratios(f);
  fc.log_ratio = f->d_r.p;
  return rc;
}
extern "C" int ppcx_fit_loo_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double* out) {
  const char* who = "ppcx_fit_loo_approx";
  std::vector<int> yenc; FitCells fc;
  int rc = loo_approx_prepare(who, f, n_genes, genes, out, yenc, fc);
  if (rc == PPCX_OK) rc = loo_approx_ratios(f, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_fit_cells(fc, kLooFields, out, loo_scratch_bytes(), f->m->stream.s));
}
extern "C" int ppcx_fit_loo_predict_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation, double p_lo,
                                           double p_hi, unsigned long long seed, double* out) {
  const char* who = "ppcx_fit_loo_predict_approx";
  std::vector<int> yenc; FitCells fc;
  int rc = loo_approx_prepare(who, f, n_genes, genes, out, yenc, fc);
  if (rc == PPCX_OK) rc = loo_predict_check_probs(p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  if (!(isfinite(truncation_compensation) && truncation_compensation > 0.0))
    return fail(PPCX_ERR_ARG, "truncation_compensation must be finite and > 0");
  if ((rc = loo_approx_ratios(f, fc)) != PPCX_OK) return rc;
  return hip_done(who, loo_predict_fit_cells(fc, truncation_compensation, p_lo, p_hi, seed32(seed), out, loo_scratch_bytes(),
                                             f->m->stream.s));
}
#ifdef PPCX_TESTING
// testing build only (ppcx_testing.h): the LOO kernel on host-given columns, on the current device
static int testing_loo(int n, int n_cols, const double* ll, const int32_t* excluded, const double* r_eff, int fields, double* out,
                       const double* log_ratio = nullptr) {
  if (n < 1 || n_cols < 1 || !ll || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  GivenCells gc;
  gc.cols = ll; gc.n = n; gc.n_cols = n_cols; gc.excl = excluded; gc.r_eff = r_eff; gc.log_ratio = log_ratio;
  const int rc = loo_reff_limits(nullptr, r_eff, n_cols, n, &gc.r_eff_min);
  if (rc != PPCX_OK) return rc;
  return hip_done(nullptr, loo_columns(gc, fields, out, loo_scratch_bytes(), nullptr));
}
extern "C" int ppcx_testing_loo(int n, int n_cols, const double* ll, const int32_t* excluded, const double* r_eff, double* out) {
  return testing_loo(n, n_cols, ll, excluded, r_eff, kLooFields, out);
}
// ... with mcse_elpd_loo and n_eff (the kernel of ppcx_fit_loo_mcse)
extern "C" int ppcx_testing_loo_mcse(int n, int n_cols, const double* ll, const int32_t* excluded, const double* r_eff, double* out) {
  return testing_loo(n, n_cols, ll, excluded, r_eff, kLooMcseFields, out);
}
// ... the kernel of ppcx_fit_loo_approx: the columns with the draws' log ratios
extern "C" int ppcx_testing_loo_approx(int n, int n_cols, const double* ll, const double* log_ratio, const int32_t* excluded, double* out) {
  if (!log_ratio) return fail(PPCX_ERR_ARG, "bad arguments");
  return testing_loo(n, n_cols, ll, excluded, nullptr, kLooFields, out, log_ratio);
}
// ... the LOO predictive kernel on host-given columns (log_ratio: as ppcx_fit_loo_predict_approx runs it)
static int testing_loo_predict(const double* ll, const double* log_ratio, const int32_t* x, int n, int n_cols, const int32_t* y,
                               const int32_t* excluded, const double* r_eff, double p_lo, double p_hi, double* out) {
  if (n < 1 || n_cols < 1 || !ll || !x || !y || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  for (size_t i = 0; i < (size_t)n * n_cols; ++i) if (x[i] < 0) return fail(PPCX_ERR_ARG, "predictive counts must be >= 0");
  GivenCells gc;
  gc.cols = ll; gc.n = n; gc.n_cols = n_cols; gc.excl = excluded; gc.r_eff = r_eff; gc.log_ratio = log_ratio;
  int rc = loo_predict_check_probs(p_lo, p_hi);
  if (rc == PPCX_OK) rc = loo_reff_limits(nullptr, r_eff, n_cols, n, &gc.r_eff_min);
  if (rc != PPCX_OK) return rc;
  return hip_done(nullptr, loo_predict_columns(gc, x, y, p_lo, p_hi, out, loo_scratch_bytes(), nullptr));
}
extern "C" int ppcx_testing_loo_predict(const double* ll, const int32_t* x, int n, int n_cols, const int32_t* y, const int32_t* excluded,
                                        const double* r_eff, double p_lo, double p_hi, double* out) {
  return testing_loo_predict(ll, nullptr, x, n, n_cols, y, excluded, r_eff, p_lo, p_hi, out);
}
extern "C" int ppcx_testing_loo_predict_approx(const double* ll, const double* log_ratio, const int32_t* x, int n, int n_cols,
                                               const int32_t* y, const int32_t* excluded, double p_lo, double p_hi, double* out) {
  if (!log_ratio) return fail(PPCX_ERR_ARG, "bad arguments");
  return testing_loo_predict(ll, log_ratio, x, n, n_cols, y, excluded, nullptr, p_lo, p_hi, out);
}
#endif
// ---- the exact posterior-predictive tails and interval of the checked genes' cells (ppcx_ppc_exact.h): every kind of fit
static int ppc_exact_check(double truncation_compensation, double p_lo, double p_hi) {
  if (!(p_lo > 0.0 && p_lo < p_hi && p_hi < 1.0)) return fail(PPCX_ERR_ARG, "need 0 < p_lo < p_hi < 1");
  if (!(isfinite(truncation_compensation) && truncation_compensation > 0.0))
    return fail(PPCX_ERR_ARG, "truncation_compensation must be finite and > 0");
  return PPCX_OK;
}
extern "C" int ppcx_fit_ppc_exact(ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation, double p_lo,
                                  double p_hi, double* out) {
  const char* who = "ppcx_fit_ppc_exact";
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  const int K = f->m->d.K;
  std::vector<int32_t> all;
  if (!genes) {                                  // all the checked genes
    if (n_genes != K) return fail(PPCX_ERR_ARG, std::string(who) + ": genes = NULL takes n_genes = K");
    all.resize((size_t)K);
    for (int i = 0; i < K; ++i) all[i] = i;
    genes = all.data();
  }
  for (int i = 0; i < n_genes; ++i) if (genes[i] < 0 || genes[i] >= K) return fail(PPCX_ERR_ARG, "gene out of range (a checked gene: 0 .. K - 1)");
  int rc = ppc_exact_check(truncation_compensation, p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  std::vector<int> yenc; FitCells fc;
  if ((rc = loo_prepare_cells(f, n_genes, genes, out, yenc, fc)) != PPCX_OK) return rc;
  return hip_done(who, ppc_exact_fit_cells(fc, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(), f->m->stream.s));
}
#ifdef PPCX_TESTING
// testing build only (ppcx_testing.h): the kernel of ppcx_fit_ppc_exact on host-given columns, on the current device
extern "C" int ppcx_testing_ppc_exact(int n, int n_cols, const double* eta, const double* sigma_raw, const int32_t* y,
                                      const int32_t* excluded, double truncation_compensation, double p_lo, double p_hi, double* out) {
  if (n < 1 || n_cols < 1 || !eta || !sigma_raw || !y || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  for (int i = 0; i < n_cols; ++i) if (y[i] < 0) return fail(PPCX_ERR_ARG, "counts must be >= 0");
  const int rc = ppc_exact_check(truncation_compensation, p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  GivenCells gc;
  gc.cols = eta; gc.n = n; gc.n_cols = n_cols; gc.excl = excluded;
  return hip_done(nullptr, ppc_exact_columns(gc, sigma_raw, y, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(), nullptr));
}
#endif
// ---- the exact leave-one-out predictive tails and interval of the checked genes' cells (ppcx_loo_exact.h): the weights of
// ppcx_fit_loo_predict / ppcx_fit_loo_predict_approx on the negative-binomial cdfs of ppcx_fit_ppc_exact
static int loo_exact_check(const ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation, double p_lo,
                           double p_hi) {
  if (!genes || n_genes < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  const int K = f->m->d.K;
  for (int i = 0; i < n_genes; ++i) if (genes[i] < 0 || genes[i] >= K) return fail(PPCX_ERR_ARG, "gene out of range (a checked gene: 0 .. K - 1)");
  return ppc_exact_check(truncation_compensation, p_lo, p_hi);
}
extern "C" int ppcx_fit_loo_predict_exact(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                          double truncation_compensation, double p_lo, double p_hi, double* out) {
  const char* who = "ppcx_fit_loo_predict_exact";
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (f->advi) return fail(PPCX_ERR_ARG, std::string(who) + " needs the draws of a NUTS fit: the exact leave-one-out intervals of "
                                                             "an ADVI fit are ppcx_fit_loo_predict_exact_approx");
  int rc = loo_exact_check(f, n_genes, genes, truncation_compensation, p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  std::vector<int> yenc; FitCells fc;
  if ((rc = loo_prepare_cells(f, n_genes, genes, out, yenc, fc)) != PPCX_OK) return rc;
  if ((rc = loo_fit_reff(who, fc, r_eff)) != PPCX_OK) return rc;
  return hip_done(who, loo_exact_fit_cells(fc, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(), f->m->stream.s));
}
extern "C" int ppcx_fit_loo_predict_exact_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double truncation_compensation,
                                                 double p_lo, double p_hi, double* out) {
  const char* who = "ppcx_fit_loo_predict_exact_approx";
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (!f->advi || !f->d_mu.p)
    return fail(PPCX_ERR_ARG, std::string(who) + " needs an ADVI fit: a NUTS fit, or one over draws produced elsewhere, holds no "
                                                 "approximation to correct for (theirs is ppcx_fit_loo_predict_exact)");
  int rc = loo_exact_check(f, n_genes, genes, truncation_compensation, p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  std::vector<int> yenc; FitCells fc;
  if ((rc = loo_approx_prepare(who, f, n_genes, genes, out, yenc, fc)) != PPCX_OK) return rc;
  if ((rc = loo_approx_ratios(f, fc)) != PPCX_OK) return rc;
  return hip_done(who, loo_exact_fit_cells(fc, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(), f->m->stream.s));
}
// ... with the cells above k_threshold matched first (ppcx_loo_mm_exact.h): ppcx_fit_loo_moment_match's kernels, then the
// predictive under their weights at the matched draws
extern "C" int ppcx_fit_loo_predict_exact_moment_match(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                                       double k_threshold, int max_iters, double truncation_compensation, double p_lo,
                                                       double p_hi, double* out) {
  const char* who = "ppcx_fit_loo_predict_exact_moment_match";
  const double probs[3] = {truncation_compensation, p_lo, p_hi};
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_mm_prepare(who, f, n_genes, genes, r_eff, k_threshold, max_iters, probs, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_mm_exact_fit_cells(fc, k_threshold, max_iters, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(),
                                              f->m->stream.s));
}
// ... and with the split transformation of the matched cells (ppcx_loo_mm_split.h step 8)
extern "C" int ppcx_fit_loo_predict_exact_moment_match_split(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                                             double k_threshold, int max_iters, double truncation_compensation,
                                                             double p_lo, double p_hi, double* out) {
  const char* who = "ppcx_fit_loo_predict_exact_moment_match_split";
  const double probs[3] = {truncation_compensation, p_lo, p_hi};
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_mm_prepare(who, f, n_genes, genes, r_eff, k_threshold, max_iters, probs, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_mm_split_fit_cells(fc, k_threshold, max_iters, true, truncation_compensation, p_lo, p_hi, out,
                                              loo_scratch_bytes(), f->m->stream.s));
}
// ... with the cells matched by the matching with the covariance step (ppcx_loo_mm_cov_exact.h): ppcx_fit_loo_moment_match_cov's
// kernels, then the predictive under their weights at the affinely matched draws; split != 0: under the split weights
extern "C" int ppcx_fit_loo_predict_exact_moment_match_cov(ppcx_fit* f, int n_genes, const int32_t* genes, const double* r_eff,
                                                           double k_threshold, int max_iters, int split,
                                                           double truncation_compensation, double p_lo, double p_hi, double* out) {
  const char* who = "ppcx_fit_loo_predict_exact_moment_match_cov";
  const double probs[3] = {truncation_compensation, p_lo, p_hi};
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_mm_prepare(who, f, n_genes, genes, r_eff, k_threshold, max_iters, probs, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_mm_cov_exact_fit_cells(fc, k_threshold, max_iters, split != 0, truncation_compensation, p_lo, p_hi, out,
                                                  loo_scratch_bytes(), f->m->stream.s));
}
// ---- gene-local moment matching of the cells of an ADVI fit with a high k-hat (ppcx_loo_mm_ap.h): the matching's kernels in
// their approximate-posterior instantiation, the ratios carrying log_p - log_g (psis_ratios), r_eff = 1
static int loo_mm_approx_prepare(const char* who, ppcx_fit* f, int n_genes, const int32_t* genes, double k_threshold, int max_iters,
                                 const double* probs, const void* out, std::vector<int>& yenc, FitCells& fc) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  int rc = loo_approx_prepare(who, f, n_genes, genes, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  if (!isfinite(k_threshold)) return fail(PPCX_ERR_ARG, std::string(who) + ": k_threshold must be finite");
  if (max_iters < 0) return fail(PPCX_ERR_ARG, std::string(who) + ": max_iters must be >= 0");
  if (probs && (rc = loo_exact_check(f, n_genes, genes, probs[0], probs[1], probs[2])) != PPCX_OK) return rc;
  return loo_approx_ratios(f, fc);
}
extern "C" int ppcx_fit_loo_moment_match_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double k_threshold, int max_iters,
                                                double* out) {
  const char* who = "ppcx_fit_loo_moment_match_approx";
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_mm_approx_prepare(who, f, n_genes, genes, k_threshold, max_iters, nullptr, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_mm_fit_cells(fc, k_threshold, max_iters, out, loo_scratch_bytes(), f->m->stream.s));
}
extern "C" int ppcx_fit_loo_predict_exact_moment_match_approx(ppcx_fit* f, int n_genes, const int32_t* genes, double k_threshold,
                                                              int max_iters, double truncation_compensation, double p_lo, double p_hi,
                                                              double* out) {
  const char* who = "ppcx_fit_loo_predict_exact_moment_match_approx";
  const double probs[3] = {truncation_compensation, p_lo, p_hi};
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_mm_approx_prepare(who, f, n_genes, genes, k_threshold, max_iters, probs, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  return hip_done(who, loo_mm_exact_fit_cells(fc, k_threshold, max_iters, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(),
                                              f->m->stream.s));
}
#ifdef PPCX_TESTING
// testing build only (ppcx_testing.h): a fit over host-given draws and host-given log ratios that the _approx entries accept -- it
// holds zeros in the approximation's place and the log ratios as psis_ratios would have cached them
extern "C" int ppcx_testing_fit_from_draws_approx(ppcx_model* m, int n_keep, const double* draws, const double* log_ratio, ppcx_fit** out) {
  if (!log_ratio) return fail(PPCX_ERR_ARG, "bad arguments");
  const int rc = ppcx_fit_from_draws(m, 1, n_keep, draws, out);
  if (rc != PPCX_OK) return rc;
  ppcx_fit* f = *out;
  f->advi = true;
  const size_t D = (size_t)m->d.D;
  hipError_t e = f->d_mu.alloc(D);
  if (e == hipSuccess) e = f->d_omega.alloc(D);
  if (e == hipSuccess) e = hipMemset(f->d_mu.p, 0, sizeof(double) * D);
  if (e == hipSuccess) e = hipMemset(f->d_omega.p, 0, sizeof(double) * D);
  if (e == hipSuccess) e = f->d_r.alloc((size_t)n_keep);
  if (e == hipSuccess) e = hipMemcpy(f->d_r.p, log_ratio, sizeof(double) * (size_t)n_keep, hipMemcpyHostToDevice);
  if (e != hipSuccess) { ppcx_fit_free(f); *out = nullptr; return fail(PPCX_ERR_HIP, hipGetErrorString(e)); }
  return PPCX_OK;
}
// testing build only (ppcx_testing.h): the kernel of ppcx_fit_loo_predict_exact and ppcx_fit_loo_predict_exact_approx on host-given
// columns, on the current device
extern "C" int ppcx_testing_loo_exact(int n, int n_cols, const double* ll, const double* eta, const double* sigma_raw, const int32_t* y,
                                      const int32_t* excluded, const double* r_eff, const double* log_ratio,
                                      double truncation_compensation, double p_lo, double p_hi, double* out) {
  if (n < 1 || n_cols < 1 || !ll || !eta || !sigma_raw || !y || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  for (int i = 0; i < n_cols; ++i) if (y[i] < 0) return fail(PPCX_ERR_ARG, "counts must be >= 0");
  if (log_ratio && r_eff) return fail(PPCX_ERR_ARG, "log_ratio takes r_eff = NULL (the draws of an approximation are independent)");
  int rc = ppc_exact_check(truncation_compensation, p_lo, p_hi);
  if (rc != PPCX_OK) return rc;
  GivenCells gc;
  gc.cols = ll; gc.n = n; gc.n_cols = n_cols; gc.excl = excluded; gc.r_eff = r_eff; gc.log_ratio = log_ratio;
  if ((rc = loo_reff_limits(nullptr, r_eff, n_cols, n, &gc.r_eff_min)) != PPCX_OK) return rc;
  return hip_done(nullptr, loo_exact_columns(gc, eta, sigma_raw, y, truncation_compensation, p_lo, p_hi, out, loo_scratch_bytes(), nullptr));
}
#endif
// ---- the relative efficiency of the same cells (loo::relative_eff(exp(log_lik), chain_id): what rstan::loo(fit) passes as r_eff)
extern "C" int ppcx_fit_relative_eff(ppcx_fit* f, int n_genes, const int32_t* genes, double* out) {
  std::vector<int> yenc; FitCells fc;
  const int rc = loo_prepare(f, n_genes, genes, out, yenc, fc);
  if (rc != PPCX_OK) return rc;
  if (f->chains > kSummaryMaxChains) return fail(PPCX_ERR_LIMIT, "ppcx_fit_relative_eff takes at most 128 chains");
  return hip_done("ppcx_fit_relative_eff", reff_fit_cells(fc, out, loo_scratch_bytes(), f->m->stream.s));
}
#ifdef PPCX_TESTING
// testing build only (ppcx_testing.h): the relative-efficiency kernel on host-given columns, on the current device
extern "C" int ppcx_testing_relative_eff(int chains, int n, int n_cols, const double* ll, double* out) {
  if (chains < 1 || n < 1 || n_cols < 1 || !ll || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  if (chains > kSummaryMaxChains) return fail(PPCX_ERR_LIMIT, "too many chains");
  GivenCells gc;
  gc.cols = ll; gc.n = (long)chains * n; gc.n_cols = n_cols; gc.chains = chains; gc.n_keep = n;
  return hip_done(nullptr, reff_columns(gc, out, loo_scratch_bytes(), nullptr));
}
#endif
extern "C" int ppcx_fit_get_diagnostics(ppcx_fit* f, double* lp, double* stepsize, int32_t* treedepth,
                                        int32_t* n_leapfrog, int32_t* divergent, double* accept) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  HIPCHK(hipSetDevice(f->m->device));
  const size_t ni = (size_t)f->chains * f->iter, nk = (size_t)f->chains * f->n_keep;
  if (lp && nk && f->d_lp.p) HIPCHK(hipMemcpy(lp, f->d_lp.p, sizeof(double) * nk, hipMemcpyDeviceToHost));
  if (stepsize && f->d_stepsize.p) HIPCHK(hipMemcpy(stepsize, f->d_stepsize.p, sizeof(double) * ni, hipMemcpyDeviceToHost));
  if (treedepth && f->d_treedepth.p) HIPCHK(hipMemcpy(treedepth, f->d_treedepth.p, sizeof(int) * ni, hipMemcpyDeviceToHost));
  if (n_leapfrog && f->d_nleap.p) HIPCHK(hipMemcpy(n_leapfrog, f->d_nleap.p, sizeof(int) * ni, hipMemcpyDeviceToHost));
  if (divergent && f->d_div.p) HIPCHK(hipMemcpy(divergent, f->d_div.p, sizeof(int) * ni, hipMemcpyDeviceToHost));
  if (accept && f->d_accept.p) HIPCHK(hipMemcpy(accept, f->d_accept.p, sizeof(double) * ni, hipMemcpyDeviceToHost));
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_inv_metric(ppcx_fit* f, double* out) {
  if (!f || !out) return fail(PPCX_ERR_ARG, "bad arguments");
  if (f->inv_metric.empty()) return fail(PPCX_ERR_ARG, "this fit has no adapted metric (not a NUTS fit)");
  memcpy(out, f->inv_metric.data(), sizeof(double) * f->inv_metric.size());
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_kernel_times(ppcx_fit* f, double* loglik_ms, double* close_ms, double* update_ms,
                                         long long* launch_triples) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (loglik_ms) *loglik_ms = f->kA_ms_mean;
  if (close_ms) *close_ms = f->kC_ms_mean;
  if (update_ms) *update_ms = f->kU_ms_mean;
  if (launch_triples) *launch_triples = f->launch_triples;
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_xchg_timing(ppcx_fit* f, double* wait_us_per_exchange, long long* exchanges) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (wait_us_per_exchange) *wait_us_per_exchange = f->xchg_count > 0 ? (double)f->xchg_ticks / 100.0 / (double)f->xchg_count : 0.0;
  if (exchanges) *exchanges = f->xchg_count;
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_ppc_timing(ppcx_fit* f, double* kernel_ms, long long* nb_draws) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (kernel_ms) *kernel_ms = f->ppc_ms;
  if (nb_draws) *nb_draws = f->ppc_draws;
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_timing(ppcx_fit* f, double* seconds, long long* grad_evals, double* gene_kernel_ms_mean,
                                   long long* gene_kernel_samples, double* gene_kernel_chain_launches_mean) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (seconds) *seconds = f->seconds;
  if (grad_evals) *grad_evals = f->grad_evals;
  if (gene_kernel_ms_mean) *gene_kernel_ms_mean = f->kA_ms_mean;
  if (gene_kernel_samples) *gene_kernel_samples = f->kA_samples;
  if (gene_kernel_chain_launches_mean) *gene_kernel_chain_launches_mean = f->kA_chain_launches_mean;
  return PPCX_OK;
}

extern "C" int ppcx_fit_ppc(ppcx_fit* f, double truncation_compensation, double p_lo, double p_hi,
                            unsigned long long seed, int n_gen, int resample, double* ci, int32_t* counts_rng) {
  if (!f || !ci) return fail(PPCX_ERR_ARG, "NULL argument");
  ppcx_model* m = f->m;
  const long n_draws = (long)f->chains * f->n_keep;
  if (n_draws < 1) return fail(PPCX_ERR_ARG, "fit holds no kept draws");
  if (m->d.K < 1) return PPCX_OK;
  if (n_gen <= 0) n_gen = (int)n_draws;
  if (!resample && n_gen > n_draws) return fail(PPCX_ERR_ARG, "n_gen exceeds the kept draws (use resample)");
  if (!(p_lo >= 0.0 && p_hi <= 1.0 && p_lo <= p_hi)) return fail(PPCX_ERR_ARG, "need 0 <= p_lo <= p_hi <= 1");
  HIPCHK(hipSetDevice(m->device));
  PpcArgs pa{};
  pa.d = m->d; pa.draws = f->d_draws.p; pa.n_draws = n_draws; pa.exposure = m->d_expo.p; pa.X = m->d_X.p;
  pa.truncation_compensation = truncation_compensation; pa.p_lo = p_lo; pa.p_hi = p_hi; pa.k0 = seed32(seed);
  pa.n_gen = n_gen; pa.resample = resample ? 1 : 0; pa.n_cells = m->d.K * m->d.S;
  float ms = -1.0f;
  const hipError_t e = ppc_fit(pa, ci, counts_rng, &ms, m->stream.s);
  if (e == hipSuccess && ms >= 0.0f) { f->ppc_ms = ms; f->ppc_draws = (long long)n_gen * pa.n_cells; }
  return hip_done(nullptr, e);
}
