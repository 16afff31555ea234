// ppcx_fit_advi.hip -- the ADVI fit, its retry wrapper, and the Pareto-k diagnostic of such a fit with the log ratios it caches
// (psis_ratios: also what the PSIS-LOO of an ADVI fit starts from, ppcx_fit_api.hip).
#include <math.h>
#include <string.h>
#include <algorithm>
#include "ppcx_host.h"
#include "ppcx_psis.h"

// ---- ADVI: mean-field variational inference, the reference's default path (rstan::vb through vb_iterative,
// R/utilities.R:246-278,1487-1494; Stan's advi.hpp algorithm restated: adapt_eta over {100,10,1,0.1,0.01},
// stochastic gradient ascent with the running-squared-gradient step, ELBO every eval_elbo iterations from
// elbo_samples draws, convergence when the mean or median of the relative ELBO changes drops below tol_rel_obj) ----
struct AdviRun {
  ppcx_model* m; Work* w; int nslot, nb_advi; uint32_t k0; uint32_t draw_id = 1; double* d_acc = nullptr; double* d_omega = nullptr;
  double lp_const = 0, ent_const = 0; int elbo_samples = 100;
};
static int advi_launch(AdviRun& r, int op, int n_slots, double eta_scaled, int first_iter, uint32_t prev_draw, uint32_t draw_base,
                       double* out_draws, int out_row0) {
  AdviArgs a;
  a.d = r.m->d; a.vecs = r.w->vecs.p; a.Dpad = r.w->Dpad; a.hyper = r.w->hyper_vecs[0].p; a.cmds = r.w->cmds[0].p; a.red = r.w->red.p;
  a.op = op; a.n_slots = n_slots; a.first_iter = first_iter; a.eta_scaled = eta_scaled; a.k0 = r.k0; a.prev_draw = prev_draw;
  a.draw_base = draw_base; a.out_draws = out_draws; a.out_row0 = out_row0; a.omega_part = r.d_omega;
  hipError_t e = launch_advi_kernel(a, r.nb_advi, r.w->stream);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("advi kernel: ") + hipGetErrorString(e));
  return PPCX_OK;
}
static int advi_eval(AdviRun& r, int n_slots) {      // gradient evaluation of the first n_slots slots
  int rc = launch_loglik(r.m, *r.w, n_slots);
  if (rc == PPCX_OK) rc = launch_close(r.m, *r.w, n_slots);
  if (rc == PPCX_OK) { RunIO io; rc = launch_step(r.m, *r.w, n_slots, io, STEP_REDUCE); }
  return rc;
}
static int advi_elbo(AdviRun& r, double* elbo) {     // Stan advi::calc_ELBO
  HIPCHK(hipMemsetAsync(r.d_acc, 0, sizeof(double) * 4, r.w->stream));
  int left = r.elbo_samples, rc;
  while (left > 0) {
    const int nb = left < r.nslot ? left : r.nslot;
    if ((rc = advi_launch(r, ADVI_DRAW, nb, 0.0, 0, 0, r.draw_id, nullptr, 0)) != PPCX_OK) return rc;
    r.draw_id += nb;
    if ((rc = advi_eval(r, nb)) != PPCX_OK) return rc;
    AdviElboArgs ea; ea.d = r.m->d; ea.cmds = r.w->cmds[0].p; ea.red = r.w->red.p; ea.n_slots = nb; ea.acc = r.d_acc;
    ea.omega_part = r.d_omega; ea.n_omega_parts = r.nb_advi;
    hipError_t e = launch_advi_elbo_kernel(ea, r.w->stream);
    if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("advi elbo kernel: ") + hipGetErrorString(e));
    left -= nb;
  }
  double acc[4];
  HIPCHK(hipMemcpyAsync(acc, r.d_acc, sizeof(acc), hipMemcpyDeviceToHost, r.w->stream));
  HIPCHK(hipStreamSynchronize(r.w->stream));
  if (acc[1] < 1.0) return fail(PPCX_ERR_INIT, "ADVI: every ELBO evaluation was non-finite");
  *elbo = acc[0] / (double)r.elbo_samples + r.lp_const * (acc[1] / (double)r.elbo_samples) + r.ent_const + acc[3];
  return PPCX_OK;
}
// draw the next gradient sample into slot 0 and evaluate it
static int advi_fresh_grad(AdviRun& r, uint32_t* id) {
  *id = r.draw_id++;
  int rc = advi_launch(r, ADVI_DRAW, 1, 0.0, 0, 0, *id, nullptr, 0);
  return rc != PPCX_OK ? rc : advi_eval(r, 1);
}
// one stochastic-gradient step (uses the gradient at draw *id), then draw + evaluate the next sample
static int advi_step(AdviRun& r, double eta, int iter_counter, uint32_t* id) {
  const uint32_t next = r.draw_id++;
  int rc = advi_launch(r, ADVI_STEP, 1, eta / sqrt((double)iter_counter), iter_counter == 1, *id, next, nullptr, 0);
  *id = next;
  return rc != PPCX_OK ? rc : advi_eval(r, 1);
}

extern "C" void ppcx_advi_config_default(ppcx_advi_config* c) {
  if (!c) return;
  c->output_samples = 1000; c->iter = 50000; c->tol_rel_obj = 0.005; c->grad_samples = 1; c->elbo_samples = 100;
  c->eval_elbo = 100; c->adapt_iter = 50; c->seed = 1; c->init_radius = 2.0;
}

extern "C" int ppcx_fit_advi(ppcx_model* m, const ppcx_advi_config* cfg, ppcx_fit** out) {
  if (!m || !cfg || !out) return fail(PPCX_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (cfg->output_samples < 1 || cfg->iter < 1 || cfg->elbo_samples < 1 || cfg->eval_elbo < 1 || cfg->adapt_iter < 1 || !(cfg->tol_rel_obj > 0))
    return fail(PPCX_ERR_ARG, "bad ADVI configuration");
  if (cfg->grad_samples != 1) return fail(PPCX_ERR_LIMIT, "grad_samples must be 1 (the reference's value)");
  HIPCHK(hipSetDevice(m->device));
  const Dims& d = m->d;
  const int D = d.D;
  AdviRun r; r.m = m;
  r.nslot = cfg->elbo_samples < 32 ? cfg->elbo_samples : 32;
  choose_launch(m, r.nslot);
  Work w; r.w = &w;
  int rc = work_alloc(w, m, r.nslot);
  if (rc != PPCX_OK) return rc;
  r.nb_advi = (D + 255) / 256; if (r.nb_advi > 1024) r.nb_advi = 1024;
  r.k0 = seed32(cfg->seed); r.elbo_samples = cfg->elbo_samples;
  const double HL2PI = 0.91893853320467274178;
  const int n2 = d.C > 2 ? d.C - 2 : 0;
  r.lp_const = -(6.0 + 2.0 * d.G + (double)n2 * d.K) * HL2PI - 5.0 * log(2.0) - (d.C >= 2 ? d.K * log(2.0) : 0.0) - (double)n2 * d.K * log(2.5);
  r.ent_const = 0.5 * (double)D * (1.0 + 2.0 * HL2PI);
  DeviceBuffer<double> acc, omega_part;          // (declared after `w`: released before it)
  HIPCHK(acc.alloc(4)); r.d_acc = acc.p;
  HIPCHK(omega_part.alloc((size_t)r.nb_advi)); r.d_omega = omega_part.p;
  hipStream_t st = w.stream;
  // ---- initial point: init = "random" U(-R, R), retried until the density and gradient are finite
  std::vector<double> q0(D), red(PT_COUNT);
  bool ok = false;
  for (int attempt = 0; attempt < 100 && !ok; ++attempt) {
    for (int i = 0; i < D; ++i) q0[i] = (2.0 * coord_uniform((uint32_t)i, (uint32_t)attempt, 0u, 0u, r.k0, 0x41445649u) - 1.0) * cfg->init_radius;
    Cmd c; cmd_clear(c); c.type = CMD_EVAL; c.dir = 1;
    for (int k = 0; k < 6; ++k) c.hyp_q[k] = q0[hyper_index(d, k)];
    c.hy = make_hyper(c.hyp_q, d.lambda_mu_mu);
    HIPCHK(hipMemcpyAsync(w.vecs.p + (size_t)V_Q1 * w.Dpad, q0.data(), sizeof(double) * D, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.cmds[0].p, &c, sizeof(Cmd), hipMemcpyHostToDevice, st));
    { RunIO io0; if ((rc = launch_update(m, w, 1, io0)) != PPCX_OK) return rc; }   // a command without a step: only the constants of the uploaded point
    if ((rc = advi_eval(r, 1)) != PPCX_OK) return rc;
    HIPCHK(hipMemcpyAsync(red.data(), w.red.p, sizeof(double) * PT_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double g6[6];
    const double lp = hyper_close(d, c.hy, c.hyp_q, red[PT_LP], red.data() + PT_H0, g6);
    ok = isfinite(lp) && red[PT_NONFINITE] == 0.0;
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(g6[k]);
  }
  if (!ok) return fail(PPCX_ERR_INIT, "ADVI: no finite initial point after 100 attempts");
  HIPCHK(hipMemcpyAsync(w.vecs.p + (size_t)V_Q0 * w.Dpad, q0.data(), sizeof(double) * D, hipMemcpyHostToDevice, st));
  {
    std::vector<double> hv((size_t)V_COUNT * 8, 0.0);
    for (int k = 0; k < 8; ++k) hv[V_MINV * 8 + k] = 1.0;
    for (int k = 0; k < 6; ++k) hv[V_Q0 * 8 + k] = q0[hyper_index(d, k)];
    HIPCHK(hipMemcpyAsync(w.hyper_vecs[0].p, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  auto reset = [&]() { return advi_launch(r, ADVI_RESET, 0, 0.0, 0, 0, 0, nullptr, 0); };
  if ((rc = reset()) != PPCX_OK) return rc;
  // ---- adapt_eta
  double elbo_init = 0, elbo_best = -INFINITY, eta_best = 0;
  if ((rc = advi_elbo(r, &elbo_init)) != PPCX_OK) return rc;
  const double eta_seq[5] = {100, 10, 1, 0.1, 0.01};
  bool tuned = false;
  for (int e = 0; e < 5 && !tuned; ++e) {
    uint32_t id;
    if ((rc = advi_fresh_grad(r, &id)) != PPCX_OK) return rc;
    for (int it = 1; it <= cfg->adapt_iter; ++it) if ((rc = advi_step(r, eta_seq[e], it, &id)) != PPCX_OK) return rc;
    double elbo = -INFINITY;
    if (advi_elbo(r, &elbo) != PPCX_OK || !isfinite(elbo)) elbo = -INFINITY;
    if (elbo < elbo_best && elbo_best > elbo_init) tuned = true;
    else if (e < 4) { elbo_best = elbo; eta_best = eta_seq[e]; }
    else { if (elbo > elbo_init) { eta_best = eta_seq[e]; tuned = true; } else return fail(PPCX_ERR_STEPSIZE, "ADVI: all proposed step-sizes failed"); }
    if ((rc = reset()) != PPCX_OK) return rc;
  }
  // ---- stochastic gradient ascent
  int cb_size = (int)fmax(0.1 * cfg->iter / cfg->eval_elbo, 2.0);
  std::vector<double> cb;
  double elbo = 0, elbo_prev = -INFINITY;
  uint32_t id;
  if ((rc = advi_fresh_grad(r, &id)) != PPCX_OK) return rc;
  int iters_done = 0; bool converged = false;
  for (int it = 1; it <= cfg->iter && !converged; ++it) {
    if ((rc = advi_step(r, eta_best, it, &id)) != PPCX_OK) return rc;
    iters_done = it;
    if (it % cfg->eval_elbo == 0) {
      elbo_prev = elbo;
      if ((rc = advi_elbo(r, &elbo)) != PPCX_OK) return rc;
      const double delta = fabs((elbo - elbo_prev) / elbo);
      cb.push_back(delta); if ((int)cb.size() > cb_size) cb.erase(cb.begin());
      double mean = 0; for (double x : cb) mean += x; mean /= cb.size();
      std::vector<double> srt(cb); std::sort(srt.begin(), srt.end());
      const double med = srt.size() % 2 ? srt[srt.size() / 2] : 0.5 * (srt[srt.size() / 2 - 1] + srt[srt.size() / 2]);
      if (mean < cfg->tol_rel_obj || med < cfg->tol_rel_obj) converged = true;
      if (!converged) { if ((rc = advi_fresh_grad(r, &id)) != PPCX_OK) return rc; }   // the ELBO draws used slot 0
    }
  }
  // ---- output_samples draws from the fitted approximation (kept as a one-chain fit)
  ppcx_fit* f = new ppcx_fit();
  fit_attach(f, m); f->chains = 1; f->n_keep = cfg->output_samples; f->iter = iters_done; f->advi = true;
  memset(&f->cfg, 0, sizeof f->cfg);
  hipError_t e = f->d_draws.alloc((size_t)cfg->output_samples * D);
  if (e == hipSuccess) e = f->d_lp.alloc_zeroed((size_t)cfg->output_samples, st);
  if (e == hipSuccess) e = f->d_stepsize.alloc_zeroed((size_t)(iters_done > 0 ? iters_done : 1), st);
  for (int row = 0; e == hipSuccess && rc == PPCX_OK && row < cfg->output_samples; row += 64) {
    const int nb = cfg->output_samples - row < 64 ? cfg->output_samples - row : 64;
    rc = advi_launch(r, ADVI_DRAW, nb, 0.0, 0, 0, r.draw_id, f->d_draws.p, row);
    r.draw_id += nb;
  }
  // the approximation itself (mu, omega of every coordinate), for the Pareto-k diagnostic (ppcx_fit_psis)
  if (e == hipSuccess) e = f->d_mu.alloc((size_t)D);
  if (e == hipSuccess) e = f->d_omega.alloc((size_t)D);
  if (e == hipSuccess && rc == PPCX_OK)
    e = launch_psis_approx_kernel(d, w.vecs.p + (size_t)V_SQ * w.Dpad, w.vecs.p + (size_t)V_SG * w.Dpad, w.hyper_vecs[0].p, f->d_mu.p, f->d_omega.p, st);
  e = finish(e, st);                             // nothing of the fit is freed under a running kernel
  if (e != hipSuccess || rc != PPCX_OK) {
    ppcx_fit_free(f);
    return rc != PPCX_OK ? rc : hip_fail(e, "the ADVI fit's draws");
  }
  f->grad_evals = (long long)r.draw_id; f->seconds = 0; f->advi_elbo = elbo; f->advi_eta = eta_best; f->advi_converged = converged ? 1 : 0;
  *out = f;
  return PPCX_OK;
}
extern "C" int ppcx_fit_advi_info(const ppcx_fit* f, int* iterations, int* converged, double* elbo, double* eta) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (iterations) *iterations = f->iter;
  if (converged) *converged = f->advi_converged;
  if (elbo) *elbo = f->advi_elbo;
  if (eta) *eta = f->advi_eta;
  return PPCX_OK;
}
// vb_iterative (R/utilities.R:246-278): rstan::vb is retried until it returns; the reference passes no seed, so every
// attempt is a fresh random start. Here attempt k runs with seed + k and the retries are bounded.
static int fit_advi_iterative(ppcx_model* m, ppcx_advi_config cfg, int max_attempts, ppcx_fit** out) {
  int rc = PPCX_ERR_ARG;
  for (int k = 0; k < max_attempts; ++k) {
    rc = ppcx_fit_advi(m, &cfg, out);
    if (rc == PPCX_OK || (rc != PPCX_ERR_INIT && rc != PPCX_ERR_STEPSIZE)) return rc;
    cfg.seed += 1;
  }
  return rc;
}
extern "C" int ppcx_fit_advi_iterative(ppcx_model* m, const ppcx_advi_config* cfg, int max_attempts, ppcx_fit** out) {
  if (!m || !cfg || !out || max_attempts < 1) return fail(PPCX_ERR_ARG, "NULL argument");
  return fit_advi_iterative(m, *cfg, max_attempts, out);
}

// ---- the Pareto-k diagnostic of an ADVI fit (rstan::vb, rstan >= 2.21: PSIS on log_p - log_g of the output draws)
static int psis_fit_check(ppcx_fit* f) {
  if (!f) return fail(PPCX_ERR_ARG, "fit is NULL");
  if (!f->advi || !f->d_mu.p) return fail(PPCX_ERR_ARG, "the Pareto-k diagnostic needs an ADVI fit (a NUTS fit, or one over draws "
                                                      "produced elsewhere, holds no approximation)");
  HIPCHK(hipSetDevice(f->m->device));            // every allocation and launch below belongs to the fit's device
  return PPCX_OK;
}
constexpr int kPsisSlots = 32;                   // draws evaluated per launch for log_p (8 .. 64 measured on cfg3)
static int psis_slots() {
#ifdef PPCX_TESTING
  if (g_test.psis_slots > 0) return g_test.psis_slots < 256 ? g_test.psis_slots : 256;   // the stage / record kernels' bound
#endif
  return kPsisSlots;
}
static size_t psis_scratch_bytes() {
#ifdef PPCX_TESTING
  if (g_test.psis_scratch_bytes > 0) return (size_t)g_test.psis_scratch_bytes;
#endif
  return kPsisScratchBytes;
}
// log_p at every kept draw through the gradient evaluation the ELBO runs (stage -> log-likelihood -> close -> reduce -> record),
// log_g and r; once per fit, cached on the device
int psis_ratios(ppcx_fit* f) {
  ppcx_model* m = f->m;
  HIPCHK(hipSetDevice(m->device));
  if (f->d_r.p) return PPCX_OK;
  const int n = f->n_keep, D = m->d.D;
  const int slots = psis_slots();
  const int nslot = n < slots ? n : slots;
  choose_launch(m, nslot);
  Work w;
  int rc = work_alloc(w, m, nslot);
  if (rc != PPCX_OK) return rc;
  DeviceBuffer<double> lp, lg, rr;               // (declared after `w`: released before it; the fit takes them on success)
  hipError_t e = lp.alloc((size_t)n);
  if (e == hipSuccess) e = lg.alloc((size_t)n);
  if (e == hipSuccess) e = rr.alloc((size_t)n);
  AdviRun r; r.m = m; r.w = &w;
  for (int row0 = 0; e == hipSuccess && rc == PPCX_OK && row0 < n; row0 += nslot) {
    const int nb = n - row0 < nslot ? n - row0 : nslot;
    e = launch_psis_stage_kernel(m->d, f->d_draws.p, row0, nb, w.vecs.p, w.Dpad, w.cmds[0].p, w.stream);
    if (e == hipSuccess && (rc = advi_eval(r, nb)) == PPCX_OK) e = launch_psis_record_kernel(m->d, w.cmds[0].p, w.red.p, nb, lp.p + row0, w.stream);
  }
  if (e == hipSuccess && rc == PPCX_OK) e = launch_psis_log_g_kernel(f->d_draws.p, n, D, f->d_mu.p, f->d_omega.p, lp.p, lg.p, rr.p, w.stream);
  e = finish(e, w.stream);
  if (rc != PPCX_OK) return rc;
  if (e != hipSuccess) return hip_fail(e, "log ratios");
  std::swap(f->d_log_p.p, lp.p); std::swap(f->d_log_g.p, lg.p); std::swap(f->d_r.p, rr.p);
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_approximation(ppcx_fit* f, double* mu, double* omega) {
  int rc = psis_fit_check(f);
  if (rc != PPCX_OK) return rc;
  const size_t bytes = sizeof(double) * (size_t)f->m->d.D;
  if (mu) HIPCHK(hipMemcpy(mu, f->d_mu.p, bytes, hipMemcpyDeviceToHost));
  if (omega) HIPCHK(hipMemcpy(omega, f->d_omega.p, bytes, hipMemcpyDeviceToHost));
  return PPCX_OK;
}
extern "C" int ppcx_fit_get_log_ratios(ppcx_fit* f, double* log_p, double* log_g) {
  int rc = psis_fit_check(f);
  if (rc == PPCX_OK) rc = psis_ratios(f);
  if (rc != PPCX_OK) return rc;
  const size_t bytes = sizeof(double) * (size_t)f->n_keep;
  if (log_p) HIPCHK(hipMemcpy(log_p, f->d_log_p.p, bytes, hipMemcpyDeviceToHost));
  if (log_g) HIPCHK(hipMemcpy(log_g, f->d_log_g.p, bytes, hipMemcpyDeviceToHost));
  return PPCX_OK;
}
extern "C" int ppcx_fit_psis(ppcx_fit* f, int n_cols, const int32_t* cols, double* khat) {
  int rc = psis_fit_check(f);
  if (rc != PPCX_OK) return rc;
  if (!cols || !khat || n_cols < 1) return fail(PPCX_ERR_ARG, "bad arguments");
  const int D = f->m->d.D;
  for (int i = 0; i < n_cols; ++i) if (cols[i] < -1 || cols[i] >= D) return fail(PPCX_ERR_ARG, "column out of range");
  if (psis_tail_len(f->n_keep) + 1 > kPsisMaxSel) return fail(PPCX_ERR_LIMIT, "ppcx_fit_psis takes at most 1.86 million draws");
  if ((rc = psis_ratios(f)) != PPCX_OK) return rc;
  hipError_t e = psis_columns(f->d_draws.p, f->d_r.p, f->n_keep, D, n_cols, cols, khat, psis_scratch_bytes(), f->m->stream.s);
  if (e != hipSuccess) return fail(PPCX_ERR_HIP, std::string("ppcx_fit_psis: ") + hipGetErrorString(e));
  return PPCX_OK;
}
#ifdef PPCX_TESTING
// testing build only (ppcx_testing.h): the PSIS kernel on host-given columns, on the current device
extern "C" int ppcx_testing_psis(int n, int n_cols, const double* lr, const double* cols, double* khat) {
  if (n < 1 || n_cols < 0 || !lr || (n_cols > 0 && !cols) || !khat) return fail(PPCX_ERR_ARG, "bad arguments");
  if (psis_tail_len(n) + 1 > kPsisMaxSel) return fail(PPCX_ERR_LIMIT, "too many draws");
  const int D = n_cols > 0 ? n_cols : 1;
  std::vector<int> ids(n_cols + 1);
  for (int i = 0; i < n_cols; ++i) ids[i] = i;
  ids[n_cols] = -1;
  DeviceBuffer<double> d_draws, d_r;
  hipError_t e = n_cols > 0 ? d_draws.upload(cols, (size_t)n * n_cols, nullptr) : d_draws.alloc((size_t)n);
  if (e == hipSuccess) e = d_r.upload(lr, (size_t)n, nullptr);
  if (e == hipSuccess) e = psis_columns(d_draws.p, d_r.p, n, D, n_cols + 1, ids.data(), khat, psis_scratch_bytes(), nullptr);
  if ((e = finish(e, nullptr)) != hipSuccess) return fail(PPCX_ERR_HIP, hipGetErrorString(e));
  return PPCX_OK;
}
#endif
