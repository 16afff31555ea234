// CPU emulation harness (TEST INFRASTRUCTURE): drives the SAME __host__ __device__ source that the
// gfx950 kernels are built from (ppcseq_amd/csrc/ppcx_{math,model,nuts,gene}.h) with plain loops in
// place of wavefront lanes and workgroups, so the host logic -- command protocol, iterative NUTS tree, adaptation --
// can be checked against the oracle without a GPU. It is never loaded by the product package.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../ppcseq_amd/csrc/ppcx_gene.h"

using namespace ppcx;

static const double* window_table() { static double t[2 * kWinTabSize]; static bool init = false; if (!init) { fill_window_log_table(t); init = true; } return t; }
static const double* log_table() { static double t[2 * kLogTabSize]; static bool init = false; if (!init) { fill_log_table(t); init = true; } return t; }

struct EmulModel {
  Dims d; int CM;
  std::vector<int> counts; std::vector<double> E, expo, X, Sy, SyE, SyX, SX, ncell, Lg1;
  std::vector<double> disp; std::vector<unsigned char> gflags; double e_min = 1.0, e_max = 1.0;     // dispersion tables (ppcx_disp.h), bit 0: excluded cells
};

static EmulModel make_model(int G, int S, int C, int K, const int32_t* counts, const double* X, const double* expo,
                            double lmm, int n_excl, const int32_t* excl) {
  EmulModel m; m.d = make_dims(G, S, C, K, lmm); m.CM = C <= 2 ? 2 : (C <= 4 ? 4 : (C <= 8 ? 8 : 16));
  m.counts.assign(counts, counts + (size_t)G * S);
  m.counts.resize((size_t)G * S + 64, 0);      // the row sweep requests counts up to two trips of 4 lanes past the end
  for (int e = 0; e < n_excl; ++e) m.counts[excl[e]] = -1;
  m.X.assign(X, X + (size_t)S * C); m.X.resize((size_t)S * C + 64, 0.0); m.expo.assign(expo, expo + S); m.E.assign(S + 64, 0.0);
  int x0 = 1;
  for (int s = 0; s < S; ++s) { m.E[s] = exp(expo[s]); if (X[s] != 1.0) x0 = 0; }
  m.e_min = m.e_max = m.E[0];
  for (int s = 1; s < S; ++s) { if (m.E[s] < m.e_min) m.e_min = m.E[s]; if (m.E[s] > m.e_max) m.e_max = m.E[s]; }
  m.d.x0_is_one = x0;
  int x1b = (C >= 2);
  for (size_t i = (size_t)S; i < (size_t)S * C && x1b; ++i) if (X[i] != 0.0 && X[i] != 1.0) x1b = 0;
  m.d.x1_binary = x1b; m.d.raw_consts = (!x0 || (C >= 2 && K > 0 && !x1b)) ? 1 : 0;
  m.Sy.assign(G, 0); m.SyE.assign(G, 0); m.SyX.assign((size_t)C * G, 0); m.SX.assign((size_t)C * G, 0); m.ncell.assign(G, 0); m.Lg1.assign(G, 0);
  m.gflags.assign(G, 0); m.disp.assign((size_t)G * kDispGeneDoubles, 0.0);
  DispFit fit; disp_fit_init(fit);
  for (int g = 0; g < G; ++g) { for (int s = 0; s < S; ++s) {
    int y = m.counts[(size_t)g * S + s]; if (y < 0) { m.gflags[g] |= 1; continue; }
    m.Sy[g] += y; m.SyE[g] += (double)y * expo[s]; m.ncell[g] += 1; m.Lg1[g] += lgamma((double)y + 1.0);
    for (int c = 0; c < C; ++c) { m.SyX[(size_t)c * G + g] += (double)y * X[(size_t)c * S + s]; m.SX[(size_t)c * G + g] += X[(size_t)c * S + s]; }
  } disp_build_gene_host(fit, m.counts.data() + (size_t)g * S, S, m.disp.data() + (size_t)g * kDispGeneDoubles); }
  return m;
}

template <int CM>
static void gene_pass(const EmulModel& m, const Cmd& c, const VecRef& v, double* red) {
  constexpr int NCM = CM + 1;
  const Dims& d = m.d;
  for (int k = 0; k < PT_COUNT; ++k) red[k] = 0.0;
  if (c.type == CMD_DONE || c.type == CMD_FLUSH) return;
  for (int g = 0; g < d.G; ++g) {
    // log-likelihood kernel (one lane per gene here)
    CellData cd; cd.counts = m.counts.data(); cd.disp = m.disp.data(); cd.gflags = m.gflags.data(); cd.Sy = m.Sy.data(); cd.ncell = m.ncell.data(); cd.e_min = m.e_min; cd.e_max = m.e_max;
    GeneSumsV<CM> o;
    lane_gene_sums<CM, 1>(d, c, v, cd, g, gene_pre_load(d, v, cd, g), 0, m.E.data(), m.expo.data(), m.X.data(), log_table(), window_table(), o);
    // close kernel
    GeneCtx<CM> x2;
    gene_load<CM>(d, c, v, g, x2);
    double pn[NCM], minv[NCM], part[10];
    gene_finish<CM>(d, c, v, x2, o, m.Sy.data(), m.SyE.data(), m.SyX.data(), m.SX.data(), m.ncell.data(), m.Lg1.data(), part, pn, minv);
    for (int k = 0; k < 10; ++k) red[k] += part[k];
    if (c.type == CMD_LEAF) { SerialSums r{red}; SlotPre<CM, 0> none; none.n = 0; leaf_close<CM, 0>(c, v, x2, pn, minv, none, r); }
  }
}
static void gene_pass_dispatch(const EmulModel& m, const Cmd& c, const VecRef& v, double* red) {
  if (m.CM == 2) gene_pass<2>(m, c, v, red);
  else if (m.CM == 4) gene_pass<4>(m, c, v, red);
  else if (m.CM == 8) gene_pass<8>(m, c, v, red);
  else gene_pass<16>(m, c, v, red);
}
// kernel B: state machine, then the per-coordinate operations of the new command; returns T0 of the gene coordinates
static double update_pass(const EmulModel& m, ChainState& st, const Cmd& ex, const double* red, double T0_prev,
                          bool have_parts, const VecRef& v, const VecRef& h, const ChainIO& io, Cmd& nc) {
  Reduced rd;
  std::vector<double> r2(red, red + PT_COUNT);
  r2[PT_T0] = T0_prev;
  chain_step(SerialLanes{}, m.d, st.sc, st.ta, ex, r2.data(), have_parts, h, io, rd, nc);
  double T0 = 0.0;
  if (nc.type != CMD_DONE)
    for (int i = 3; i < m.d.off_tail; ++i) coord_update(m.d, nc, v, i, io.draws, &T0);
  return T0;
}

struct EmulCfg { int chains, iter, warmup; unsigned long long seed; double adapt_delta; int max_treedepth;
                 double init_radius, stepsize0; int init_buffer, term_buffer, window, chain_id_offset; };

static NutsConfig nuts_config(const EmulCfg& cfg) {
  NutsConfig nc;
  nc.chains = cfg.chains; nc.iter = cfg.iter; nc.warmup = cfg.warmup; nc.seed = cfg.seed;
  nc.adapt_delta = cfg.adapt_delta; nc.max_treedepth = cfg.max_treedepth; nc.init_radius = cfg.init_radius;
  nc.stepsize0 = cfg.stepsize0; nc.init_buffer = cfg.init_buffer; nc.term_buffer = cfg.term_buffer;
  nc.window = cfg.window; nc.chain_id_offset = cfg.chain_id_offset;
  return nc;
}
// chain ch's part of the fits' output arrays: draws [chains][nk][D], lp [chains][nk], diagnostics [chains][iter]
static ChainIO chain_io(int ch, int nk, int D, int iter, double* draws, double* lp, double* stepsize, int* treedepth,
                        int* n_leapfrog, int* divergent, double* accept) {
  ChainIO io;
  io.draws = draws + (size_t)ch * nk * D;
  io.out.lp = lp + (size_t)ch * nk; io.out.stepsize = stepsize + (size_t)ch * iter;
  io.out.treedepth = treedepth + (size_t)ch * iter; io.out.n_leapfrog = n_leapfrog + (size_t)ch * iter;
  io.out.divergent = divergent + (size_t)ch * iter; io.out.accept = accept + (size_t)ch * iter;
  return io;
}

// where the fits below leave each chain's inverse metric at its end ([chains][D], gene and hyper coordinates; null: nowhere)
static double* g_minv_out = nullptr;
extern "C" __attribute__((visibility("default")))
void emul_set_inv_metric_out(double* out) { g_minv_out = out; }
static void store_inv_metric(const EmulModel& m, int ch, const std::vector<double>& vecs, const std::vector<double>& hv) {
  if (!g_minv_out) return;
  const int D = m.d.D;
  double* o = g_minv_out + (size_t)ch * D;
  for (int i = 0; i < D; ++i) o[i] = vecs[(size_t)V_MINV * D + i];
  for (int k = 0; k < 6; ++k) o[hyper_index(m.d, k)] = hv[V_MINV * 8 + k];   // the hyper coordinates live in their own copy
}

extern "C" __attribute__((visibility("default")))
int emul_log_prob_grad(int G, int S, int C, int K, const int32_t* counts, const double* X, const double* expo,
                       double lmm, int n_excl, const int32_t* excl, const double* u, double* lp, double* grad) {
  EmulModel m = make_model(G, S, C, K, counts, X, expo, lmm, n_excl, excl);
  const int D = m.d.D;
  std::vector<double> vecs((size_t)V_COUNT * D, 0.0), hv((size_t)V_COUNT * 8, 0.0), red(PT_COUNT, 0.0);
  for (int i = 0; i < D; ++i) { vecs[(size_t)V_Q1 * D + i] = u[i]; vecs[(size_t)V_MINV * D + i] = 1.0; }
  for (int k = 0; k < 6; ++k) { hv[V_Q1 * 8 + k] = u[hyper_index(m.d, k)]; hv[V_MINV * 8 + k] = 1.0; }
  EmulCfg one; memset(&one, 0, sizeof one); one.chains = 1; one.max_treedepth = 10; one.adapt_delta = 0.8; one.init_radius = 2; one.stepsize0 = 1;
  const NutsConfig nc = nuts_config(one);
  ChainState st; state_init(st, nc, 0, 1);
  Cmd c, n; cmd_clear(c);
  ChainIO io; memset(&io, 0, sizeof io);
  VecRef v{vecs.data(), D}, h{hv.data(), 8};
  double T0 = update_pass(m, st, c, red.data(), 0.0, false, v, h, io, n); c = n;
  while (c.type != CMD_DONE) {
    gene_pass_dispatch(m, c, v, red.data());
    T0 = update_pass(m, st, c, red.data(), T0, true, v, h, io, n); c = n;
  }
  *lp = st.sc.lp_eval;
  for (int i = 0; i < D; ++i) grad[i] = vecs[(size_t)V_G1 * D + i];
  for (int k = 0; k < 6; ++k) grad[hyper_index(m.d, k)] = hv[V_G1 * 8 + k];
  return 0;
}

// draws [chains][n_keep][D]; lp [chains][n_keep]; diagnostics [chains][iter]
extern "C" __attribute__((visibility("default")))
int emul_fit_nuts(int G, int S, int C, int K, const int32_t* counts, const double* X, const double* expo, double lmm,
                  int n_excl, const int32_t* excl, const EmulCfg* cfg, double* draws, double* lp, double* stepsize,
                  int* treedepth, int* n_leapfrog, int* divergent, double* accept) {
  EmulModel m = make_model(G, S, C, K, counts, X, expo, lmm, n_excl, excl);
  const int D = m.d.D, nk = cfg->iter - cfg->warmup;
  const NutsConfig nc = nuts_config(*cfg);
  int rc = 0;
  for (int ch = 0; ch < cfg->chains; ++ch) {
    std::vector<double> vecs((size_t)V_COUNT * D, 0.0), hv((size_t)V_COUNT * 8, 0.0), red(PT_COUNT, 0.0);
    for (int i = 0; i < D; ++i) vecs[(size_t)V_MINV * D + i] = 1.0;
    for (int k = 0; k < 8; ++k) hv[V_MINV * 8 + k] = 1.0;
    ChainState st; state_init(st, nc, ch, 0);
    Cmd c, n; cmd_clear(c);
    const ChainIO io = chain_io(ch, nk, D, cfg->iter, draws, lp, stepsize, treedepth, n_leapfrog, divergent, accept);
    VecRef v{vecs.data(), D}, h{hv.data(), 8};
    double T0 = update_pass(m, st, c, red.data(), 0.0, false, v, h, io, n); c = n;
    long guard = 0;
    while (c.type != CMD_DONE) {
      gene_pass_dispatch(m, c, v, red.data());
      T0 = update_pass(m, st, c, red.data(), T0, true, v, h, io, n); c = n;
      if (++guard > 50000000L) { rc = -5; break; }
    }
    if (st.sc.error) rc = -3;
    store_inv_metric(m, ch, vecs, hv);
  }
  return rc;
}

// ---- pipelined rounds (ppcx_ls_kernel + ppcx_gene_kernel on the device): the same protocol with plain loops.
// ls_first_s: run the state machine before the log-likelihood part of the merged launch (on the device they run side by
// side: neither may depend on the other, so both orders must give the same chain).
template <int CM>
static void pipelined_loglik(const EmulModel& m, const Cmd& x, const VecRef& v, std::vector<GeneSumsV<CM>>& sums) {
  if (x.type == CMD_DONE || x.type == CMD_FLUSH) return;
  if (x.evaluated && x.type != CMD_LEAF) return;               // closed, and nothing was anticipated after it
  CellData cd; cd.counts = m.counts.data(); cd.disp = m.disp.data(); cd.gflags = m.gflags.data(); cd.Sy = m.Sy.data(); cd.ncell = m.ncell.data(); cd.e_min = m.e_min; cd.e_max = m.e_max;
  for (int g = 0; g < m.d.G; ++g)
    lane_gene_sums<CM, 1>(m.d, x, v, cd, g, gene_pre_load(m.d, v, cd, g), 0, m.E.data(), m.expo.data(), m.X.data(), log_table(), window_table(), sums[g]);
}
template <int CM>
static void pipelined_gene(const EmulModel& m, const Cmd& y, const VecRef& v, double* draws, bool spec,
                           std::vector<GeneSumsV<CM>>& sums, double* red) {
  constexpr int NCM = CM + 1;
  const Dims& d = m.d;
  if (y.type == CMD_DONE) return;
  const bool do_update = !y.updated, do_close = y.evaluated && y.type != CMD_FLUSH;
  if (do_close) for (int k = 0; k < PT_COUNT; ++k) if (k != PT_T0) red[k] = 0.0;
  double T0 = 0.0;
  for (int g = 0; g < d.G; ++g) {
    GeneCtx<CM> x;
    gene_index<CM>(d, g, x);
    if (do_update) gene_coord_update<CM>(d, y, v, x, draws, &T0, !do_close);
    if (!do_close) continue;
    if (do_update) gene_params<CM>(d, v, x); else gene_load<CM>(d, y, v, g, x);
    double pn[NCM], minv[NCM], gn[NCM], part[10];
    GeneSumsV<CM> o = sums[g];
    gene_finish<CM>(d, y, v, x, o, m.Sy.data(), m.SyE.data(), m.SyX.data(), m.SX.data(), m.ncell.data(), m.Lg1.data(), part, pn, minv, gn);
    for (int k = 0; k < 10; ++k) if (k != PT_T0) red[k] += part[k];
    if (y.type == CMD_LEAF) {
      SerialSums r{red}; SlotPre<CM, 0> none; none.n = 0;
      leaf_close<CM, 0>(y, v, x, pn, minv, none, r);
      if (spec) gene_spec_consts<CM>(d, y, v, x, pn, gn, minv);
    }
  }
  if (do_update) red[PT_T0] = T0;
}
template <int CM>
static int pipelined_chain(const EmulModel& m, const NutsConfig& nc, int ch, const ChainIO& io, bool spec, bool ls_first_s,
                           long* rounds, long* carried) {
  const int D = m.d.D;
  std::vector<double> vecs((size_t)V_COUNT * D, 0.0), hv((size_t)V_COUNT * 8, 0.0), red(PT_COUNT, 0.0);
  for (int i = 0; i < D; ++i) vecs[(size_t)V_MINV * D + i] = 1.0;
  for (int k = 0; k < 8; ++k) hv[V_MINV * 8 + k] = 1.0;
  std::vector<GeneSumsV<CM>> sums(m.d.G);
  ChainState st; state_init(st, nc, ch, 0);
  Cmd x, y; cmd_clear(x);
  VecRef v{vecs.data(), D}, h{hv.data(), 8};
  Reduced rd;
  for (long guard = 0; guard < 100000000L; ++guard) {
    if (!ls_first_s) pipelined_loglik<CM>(m, x, v, sums);
    const Cmd x_seen = x;                                         // what the log-likelihood part of the launch reads
    const bool stepped = chain_step_pipelined(SerialLanes{}, m.d, st.sc, st.ta, x, red.data(), h, io, rd, y, spec);
    if (ls_first_s) pipelined_loglik<CM>(m, x_seen, v, sums);
    ++*rounds; if (!stepped) ++*carried;
    x = y;
    if (x.type == CMD_DONE) { store_inv_metric(m, ch, vecs, hv); return st.sc.error ? -3 : 0; }
    pipelined_gene<CM>(m, x, v, io.draws, spec, sums, red.data());
  }
  return -5;
}
// rounds[chains], carried[chains]: launches per chain and how many of them only carried a command (mis-anticipations)
extern "C" __attribute__((visibility("default")))
int emul_fit_nuts_pipelined(int G, int S, int C, int K, const int32_t* counts, const double* X, const double* expo, double lmm,
                            int n_excl, const int32_t* excl, const EmulCfg* cfg, int spec, int ls_first_s, double* draws, double* lp,
                            double* stepsize, int* treedepth, int* n_leapfrog, int* divergent, double* accept, long* rounds,
                            long* carried) {
  EmulModel m = make_model(G, S, C, K, counts, X, expo, lmm, n_excl, excl);
  const int D = m.d.D, nk = cfg->iter - cfg->warmup;
  const NutsConfig nc = nuts_config(*cfg);
  int rc = 0;
  for (int ch = 0; ch < cfg->chains; ++ch) {
    const ChainIO io = chain_io(ch, nk, D, cfg->iter, draws, lp, stepsize, treedepth, n_leapfrog, divergent, accept);
    rounds[ch] = 0; carried[ch] = 0;
    int r;
    if (m.CM == 2) r = pipelined_chain<2>(m, nc, ch, io, spec != 0, ls_first_s != 0, rounds + ch, carried + ch);
    else if (m.CM == 4) r = pipelined_chain<4>(m, nc, ch, io, spec != 0, ls_first_s != 0, rounds + ch, carried + ch);
    else if (m.CM == 8) r = pipelined_chain<8>(m, nc, ch, io, spec != 0, ls_first_s != 0, rounds + ch, carried + ch);
    else r = pipelined_chain<16>(m, nc, ch, io, spec != 0, ls_first_s != 0, rounds + ch, carried + ch);
    if (r != 0) rc = r;
  }
  return rc;
}

// the dispersion table of one row (ppcx_disp.h): Fh and Dh at the given sigma_raw -- by table lookup (in[i] = 1) or, outside
// the tabulated range, by the direct evaluation that also builds the table; direct[] always holds the direct evaluation
extern "C" __attribute__((visibility("default")))
int emul_disp_table(const int32_t* row, int S, int n, const double* sigma, double* F, double* D, double* F_direct, double* D_direct, int* in) {
  DispFit fit; disp_fit_init(fit);
  std::vector<double> t(kDispGeneDoubles);
  disp_build_gene_host(fit, row, S, t.data());
  for (int i = 0; i < n; ++i) {
    const DispRef r = disp_ref(sigma[i]);
    const DispPoint pt = disp_point(sigma[i]);
    disp_row(row, S, 0, 1, pt, &F_direct[i], &D_direct[i]);
    in[i] = r.in ? 1 : 0;
    if (r.in) {
      const double* pc = t.data() + (long)r.panel * 2 * kDispStride;
      F[i] = disp_horner(pc, r.x); D[i] = disp_horner(pc + kDispStride, r.x);
    } else { F[i] = F_direct[i]; D[i] = D_direct[i]; }
  }
  return 0;
}

extern "C" __attribute__((visibility("default")))
int emul_nb2_log_rng(double eta, double phi, unsigned long long seed, unsigned cell, unsigned draw) {
  return nb2_log_rng(eta, phi, seed32(seed), cell, draw);
}

// draws 0 .. n - 1 of one cell's stream (tests/test_nb_rng_distribution.py: 20 000 draws per designed point)
extern "C" __attribute__((visibility("default")))
int emul_nb2_log_rng_draws(double eta, double phi, unsigned long long seed, unsigned cell, int n, int32_t* out) {
  for (int j = 0; j < n; ++j) out[j] = nb2_log_rng(eta, phi, seed32(seed), cell, (unsigned)j);
  return 0;
}

// the host twin of the testing build's ppcx_testing_eval_math (ppcseq_amd/csrc/ppcx_testing_math.hip): the same functions and
// function ids (ppcx_testing.h PPCX_MATH_*), here their #else branches
extern "C" __attribute__((visibility("default")))
int emul_eval_math(int fn, int n, const double* a, const double* b, const int32_t* y, double* out0, double* out1) {
  GeneParams<2> gp;
  gp.coef[0] = gp.coef[1] = 0.0; gp.sigma_raw = 0.0; gp.phi = 1.0; gp.invphi = 1.0;
  for (int i = 0; i < n; ++i) {
    const double x = a[i], x2 = b[i];
    double r0 = 0.0, r1 = 0.0;
    CellAcc<2> acc; acc.zero();
    switch (fn) {
      case 0: r0 = fast_rcp(x); break;
      case 1: r0 = fast_log(x); break;
      case 2: r0 = fast_exp(x); break;
      case 3: r0 = table_log(x, log_table()); break;
      case 4: r0 = window_log(x, window_table()); break;
      case 5: stirling_tails(x, &r0, &r1); break;
      case 6: stirling_excess(x, x2, log_table(), y[i] != 0, &r0, &r1); break;
      case 7: log_erfc_and_ratio(x, &r0, &r1); break;
      case 8: (void)cell_eval<2, false>(y[i], x, x2, gp, log_table(), acc); r0 = acc.SL; r1 = acc.Sq; break;
      case 9: (void)cell_eval_win<2, false>(y[i], x, x2, 1.0, gp, window_table(), acc); r0 = acc.SL; r1 = acc.Sq; break;
      case 10: (void)cell_eval<2, false>(y[i], x, x2, gp, log_table(), acc); r0 = acc.SA; r1 = acc.SYq; break;
      case 11: (void)cell_eval_win<2, false>(y[i], x, x2, 1.0, gp, window_table(), acc); r0 = acc.SA; r1 = acc.SYq; break;
      case 12: sincos_2pi(x, &r0, &r1); break;
      case 13: r0 = lgamma_int1(x); break;
      case 14: r0 = rng_exp(x); break;
      case 15: r0 = rng_div(x, x2); break;
      default: return -1;
    }
    out0[i] = r0; out1[i] = r1;
  }
  return 0;
}

// the dispersion table of one row as the host builds it (kDispGeneDoubles doubles, ppcx_disp.h layout)
extern "C" __attribute__((visibility("default")))
int emul_disp_build(const int32_t* row, int S, double* out) {
  DispFit fit; disp_fit_init(fit);
  disp_build_gene_host(fit, row, S, out);
  return 0;
}
