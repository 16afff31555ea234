"""The device's building blocks at their edges, one element at a time, and the gene-level paths that sit on those edges.

1. ppcx_math.h and the cells of ppcx_model.h on the device (the testing build's ppcx_testing_eval_math: gfx950 branches, the
   cells' assembly, the log tables in LDS) against mpmath at 40 digits, on the grids and bounds of tests/math_edges.py.
2. The dispersion tables that ppcx_disp_build_kernel builds on the device, read back: equal to the host build coefficient by
   coefficient, and evaluated at the panel edges against mpmath.
3. Through the public ppcx_log_prob_grad, small models against the oracle at every lanes-per-gene value: sigma_raw on the
   table's panel edges and ends, a gene's window limits (ppcx_model.h gene_window) in the three factorised modes, and the
   skew-normal prior where erfc underflows.
Bounds of part 3: lp within 1e-12 relative, each gradient coordinate within 1e-11 (1 + |g_o|) -- ten times tighter than
tests/test_gpu_parity.py."""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

from tests import math_edges as me
from tests.emul_util import P
from tests.gpu_fixtures import testing_library
from tests.test_disp_table import _exact, _rows

pytestmark = pytest.mark.gpu

LANES = (1, 2, 4, 8, 16, 64)
LP_TOL, G_TOL = 1e-12, 1e-11


@pytest.fixture(scope="module")
def L():
    with testing_library() as _lib:
        if _lib.device_count() < 1:
            pytest.fail("no HIP device visible: the product has no CPU fallback")
        yield _lib


# ---- 1. the building blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(me.CHECKS))
def test_device_math_edges_match_mpmath(L, name):
    me.CHECKS[name](L.testing_eval_math)


# ---- 2. the dispersion tables the device builds --------------------------------------------------------------------------
def _table_rows():
    rows = dict(_rows())
    S = rows["low"].size
    rows["tiers"] = np.resize(np.array([7, 8, 31, 32, 255, 256], np.int32), S)     # the y < 8 / Stirling switch, 32, 256
    rows["allzero"] = np.zeros(S, np.int32)
    ex = rows["high"].copy(); ex[[0, 5, S - 1]] = -1
    rows["excluded_high"] = ex
    return rows


def _horner_fma(c, x):
    """ppcx_disp.h disp_horner: Horner's recurrence in multiply-adds (one rounding per step)"""
    p = float(c[-1])
    with mp.workdps(60):
        for k in range(len(c) - 2, -1, -1):
            p = float(mp.mpf(p) * mp.mpf(float(x)) + mp.mpf(float(c[k])))
    return p


def test_device_dispersion_tables_match_host_and_mpmath(L, emul):
    rows = _table_rows()
    names = list(rows)
    S = rows[names[0]].size
    cnt = np.stack([rows[k] for k in names])
    excl = np.flatnonzero(cnt.ravel() < 0).astype(np.int32)
    m = L.Model(np.maximum(cnt, 0), np.ones((S, 1)), np.zeros(S), 0, excl=excl)
    try:
        dev = m.testing_disp_table()
    finally:
        m.close()
    for gi, name in enumerate(names):
        row = np.ascontiguousarray(cnt[gi], np.int32)
        host = np.zeros(768)
        emul.emul_disp_build(P(row, C.c_int32), S, P(host, C.c_double))
        host = host.reshape(32, 2, 12)
        # the polynomials as functions, to 1e-15 of their size on the panel (the sum of |coefficients| bounds them on [-1, 1]),
        # at 65 points of every panel
        size = np.sum(np.abs(host), axis=2)
        xs = np.cos(np.pi * np.arange(65) / 64)
        pv = lambda t: np.stack([np.polynomial.polynomial.polyval(xs, t[p, f, :11]) for p in range(32) for f in (0, 1)])  # noqa: E731
        dv = np.abs(pv(dev[gi]) - pv(host))
        assert np.all(dv <= 1e-15 * size.reshape(-1, 1)), (name, "values", np.max(dv / np.maximum(size.reshape(-1, 1), 1e-300)))
        # coefficient by coefficient: the monomial form amplifies the node values' last bits (2^(k-1) for x^k: 1e-13 of the size
        # at the high degrees)
        dc = np.abs(dev[gi] - host)
        assert np.all(dc <= 4e-13 * size[:, :, None]), (name, "coefficients", np.max(dc / np.maximum(size[:, :, None], 1e-300)))
        # the device's table at the panel edges (and 1e-3 inside / outside them), evaluated as the kernels look it up
        for j in range(33):
            b = -8.0 + 0.5 * j
            for sg in (np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf), b - 1e-3, b + 1e-3):
                t = (sg + 8.0) * 2.0
                if not 0.0 <= t < 32.0:
                    continue
                p = int(t)
                x = (sg - (-8.0 + 0.5 * p)) * 4.0 - 1.0
                vals = [_horner_fma(dev[gi, p, f, :11], x) for f in (0, 1)]
                eF, eD = _exact(row, float(sg))
                for got, ex in zip(vals, (eF, eD)):
                    # test_disp_table's bound for the host build (8e-16 |value| + 1e-13) and 2e-16 |value| for the device's node
                    # values, whose fast_exp / fast_rcp differ from the host's in the last bit (worst measured: 8.3e-16 |value|,
                    # row "mid", Dh at sigma = 6 - ulp, where the host build is at 6.8e-16)
                    assert abs(got - float(ex)) <= 1e-15 * float(abs(ex)) + 1e-13, (name, sg, got, float(ex))


# ---- 3. gene-level edges through ppcx_log_prob_grad ------------------------------------------------------------------------
def _compare(L, oracle, counts, X, expo, K, U, what):
    mo = oracle.model(counts, X, expo, K)
    ref = [oracle.log_prob_grad(mo, U[i]) for i in range(U.shape[0])]
    m = L.Model(counts, X, expo, K)
    try:
        for lanes in LANES:
            m.set_launch(lanes, 0)
            lp, g = m.log_prob_grad(U)
            for i in range(U.shape[0]):
                lpo, go = ref[i]
                assert np.isfinite(lpo), (what, i)
                assert abs(lp[i] - lpo) <= LP_TOL * abs(lpo), (what, lanes, i, lp[i], lpo)
                e = np.abs(g[i] - go) / (1 + np.abs(go))
                assert np.max(e) <= G_TOL, (what, lanes, i, int(np.argmax(e)), g[i][np.argmax(e)], go[np.argmax(e)])
    finally:
        m.close()
    return ref


def _base(G, S, C, K, seed):
    from oracle import independent as ind
    rng = np.random.default_rng(seed)
    counts = rng.negative_binomial(5.0, 5.0 / (5.0 + rng.uniform(2, 400, (G, 1))), (G, S)).astype(np.int32)
    o = ind.offsets(G, C, K)
    u = rng.uniform(-0.5, 0.5, o["D"])
    return counts, o, u


def test_sigma_raw_on_dispersion_panel_edges(L, oracle):
    """sigma_raw of each gene on a panel boundary and next to it, the table's ends and the first direct evaluation: the lanes'
    chunked Horner of the panel (ppcx_gene.h lane_gene_sums) and disp_row_at beside it"""
    G, S = 6, 40
    counts, o, u0 = _base(G, S, 1, 0, 21)
    counts[1] = np.resize([7, 8, 31, 32, 255, 256], S)
    counts[2] = 0
    sig = []
    for j in range(33):
        b = -8.0 + 0.5 * j
        sig += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)]
    sig = np.array(sig)
    rows = -(-sig.size // G)
    U = np.tile(u0, (rows, 1))
    U[:, 3:3 + G] += 4.0
    for i in range(rows):
        for g in range(G):
            U[i, o["sigma_raw"] + g] = sig[(i * G + g) % sig.size]
    _compare(L, oracle, counts, np.ones((S, 1)), np.linspace(-0.3, 0.3, S), 0, U, "panel edges")


def _neighbours(p0, n):
    out = [p0]
    lo = hi = p0
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out = [lo] + out + [hi]
    return np.array(out)


def _fma1(e, a):
    with mp.workdps(60):
        return float(mp.mpf(float(e)) * mp.mpf(float(a)) + 1)


def _pick(vals, T):
    """the two steps whose bound lies nearest below T and the two nearest at or above it (on the double below T and on T
    itself where the steps reach them)"""
    below, above = np.flatnonzero(vals < T), np.flatnonzero(vals >= T)
    assert below.size >= 2 and above.size >= 2, "the steps do not straddle the target"
    return sorted(set(below[np.argsort(T - vals[below])[:2]]) | set(above[np.argsort(vals[above] - T)[:2]]))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gene_window_limits(L, oracle, mode):
    """a gene's w_max on 2^(k+4) - ulp and 2^(k+4), its w_min on 2^k - ulp and 2^k (k = 2): the windowed cell on one side, the
    general cell on the other (ppcx_model.h gene_window). The gene has sigma_raw = 0, so that its A = exp(intercept) is the
    device's fast_exp of the intercept exactly (read back through the testing build) and the window's bounds can be placed on
    the double; MODE 1 moves A1 = A exp(alpha_1) across the limit, MODE 2 (C = 4 indicator columns) a_hi = A exp(alpha_2)"""
    G, S = 4, 24
    C = {0: 1, 1: 2, 2: 4}[mode]
    K = 0 if mode == 0 else 1
    counts, o, u0 = _base(G, S, C, K, 30 + mode)
    expo = np.linspace(0.0, math.log(12.0), S)            # E_s from 1 to 12 (e_min = exp(0) = 1 exactly)
    e_min = math.exp(expo[0]); e_max = math.exp(expo[-1])
    X = np.ones((S, C))
    if C >= 2:
        X[:, 1] = np.arange(S) % 2
    if C == 4:
        X[:, 2] = (np.arange(S) % 3 == 0); X[:, 3] = (np.arange(S) % 4 == 1)
    u0[3:3 + G] = -3.0                                    # the other genes: w in [1.05, 1.6], windowed
    u0[o["sigma_raw"]:o["sigma_raw"] + G] = 0.0
    u0[o["alpha1"]:o["alpha2"]] = 0.0
    u0[o["alpha2"]:o["sigma_raw"]] = 0.0
    fe = lambda v: L.testing_eval_math("fast_exp", v)[0]  # noqa: E731
    rows = []
    for bound, T in (("max", 64.0), ("min", 4.0)):
        # target: (w at the gene constant being stepped) = T, with the other end of the window inside the four binades
        if mode == 0:
            Ahat = (T - 1) / (e_max if bound == "max" else e_min)
            steps = _neighbours(math.log(Ahat), 48)
            A = fe(steps)
            vals = np.array([_fma1(e_max if bound == "max" else e_min, a) for a in A])
            for i in _pick(vals, T):
                u = u0.copy(); u[3] = steps[i]; rows.append(u)
        else:
            A_fixed = 4.4 if bound == "max" else 4.0          # w of the unmoved constant: [5.4, 53.8] / [5, 49]
            icpt = math.log(A_fixed)
            A = fe(np.array([icpt]))[0]
            target = (T - 1) / (e_max if bound == "max" else e_min) / A
            steps = _neighbours(math.log(target), 48)
            ec = fe(steps)
            a_moved = A * ec                                  # A1 = A exp(alpha_1) (MODE 1); a_hi or a_lo = A exp(alpha_2_1) (MODE 2)
            vals = np.array([_fma1(e_max if bound == "max" else e_min, a) for a in a_moved])
            for i in _pick(vals, T):
                u = u0.copy(); u[3] = icpt
                u[o["alpha1"] if mode == 1 else o["alpha2"]] = steps[i]
                rows.append(u)
    assert len(rows) >= 8
    _compare(L, oracle, counts, X, expo, K, np.array(rows), f"window mode {mode}")


def test_skew_normal_prior_where_erfc_underflows(L, oracle):
    """one gene's x = -lambda_skew z / sqrt 2 at 26.40 ... 26.65 (ppcx_math.h log_erfc_and_ratio): the intercept's gradient
    and the three hyper-gradients the skew-normal prior feeds (lambda_mu, lambda_sigma, lambda_skew)"""
    G, S = 3, 16
    counts, o, u0 = _base(G, S, 1, 0, 41)
    expo = np.linspace(-0.2, 0.2, S)
    lmm = 5.612671
    u0[1] = 0.0                                           # omega = 1 exactly
    lam = -5.0
    u0[2] = lam
    xi = u0[0] + 2 * lmm
    u0[3:3 + G] = xi + 0.1
    rows = []
    for xt in (26.40, 26.46, 26.50, 26.60, 26.65):
        u = u0.copy()
        u[3] = xi + xt * math.sqrt(2.0) / -lam            # z = x sqrt 2 / -lambda
        rows.append(u)
    U = np.array(rows)
    ref = _compare(L, oracle, counts, np.ones((S, 1)), expo, 0, U, "skew edge")
    # the coordinates the ratio feeds, on their own (the comparison above covers them at the same bound)
    m = L.Model(counts, np.ones((S, 1)), expo, 0)
    try:
        _, g = m.log_prob_grad(U)
    finally:
        m.close()
    for i in range(U.shape[0]):
        for c in (0, 1, 2, 3):
            assert abs(g[i][c] - ref[i][1][c]) <= G_TOL * (1 + abs(ref[i][1][c])), (i, c, g[i][c], ref[i][1][c])
