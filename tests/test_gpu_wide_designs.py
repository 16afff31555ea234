"""The per-cell statistics on designs with more than one slope, on the device: the draw sets of tests/wide_design_cases.py (C = 3
with a continuous covariate, C = 4 with three indicators; three genes, two of them checked) reach the kernels through
Model.fit_from_draws. Fit.loo_moment_match and Fit.loo_predict_exact_moment_match, plain and split, are held to the CPU builds of
their headers on the designed cells; the draw counts of the C = 4 set run with the gene table and the cell scratch both in
batches; Fit.log_lik, Fit.loo, Fit.ppc_exact and Fit.loo_predict_exact are held to scipy and to their restatements with eta
formed in numpy for any C; gene subsets, permuted gene lists and second calls give the same bits.

Tolerances: iterations and the other integer fields equal, NaN and Inf in the same places, a cell with iterations == 0 bit-equal
to Fit.loo; the reals against the CPU builds at ten times the largest error measured on these cells in units of max(1, |ref|)
(W.WIDE_GPU_MEASURED, one value per test; each test prints its own), never above 1e-9. The fit-level statistics: the tolerances
of tests/test_gpu_loo.py, tests/test_gpu_ppc_exact.py and tests/test_gpu_loo_exact.py. tests/test_wide_designs_host.py holds the
CPU builds to the restatements on the same cells."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as S
from tests import loo_restate as L
from tests import ppc_exact_restate as E
from tests import wide_design_cases as W
from tests.gpu_fixtures import testing_library
from tests.test_gpu_loo import _compare, _reference_ll
from tests.test_gpu_loo_mm import _Held, _against_host as _mm_against, _row as _mm_row
from tests.test_gpu_loo_mm_exact import _against_host as _exact_against_host
from tests.test_gpu_loo_mm_split import _against_host as _split_against, _exact_against, _row as _split_row

pytestmark = pytest.mark.gpu

TC = 0.7352941
MM_KEYS = R.HEAD + ("scale", "shift")
SPLIT_KEYS = MM_KEYS + S.TAIL
XKEYS = X.HEAD + ("scale", "shift", "pit_lt", "pit_le")
SETS = ("covariate", "factor4")


def _bound(what):
    return min(10 * W.WIDE_GPU_MEASURED[what], W.BOUND)


@pytest.fixture(scope="module")
def mm_host():
    return R.host_lib()


@pytest.fixture(scope="module")
def exact_host():
    return X.host_lib()


@pytest.fixture(scope="module")
def split_host():
    return S.host_lib()


@pytest.fixture(scope="module")
def held():
    """the two wide draw sets as models and fits of the product library"""
    h = {}
    try:
        for name in SETS:
            h[name] = _Held(W.draw_set(name))
        yield h
    finally:
        for x in h.values():
            x.close()


def _column_batch(scratch_bytes, rows, n_cols):
    """column_batch of ppcx_columns.h: columns of `rows` doubles under the bound, at least one, at most all"""
    return min(max(1, scratch_bytes // (8 * rows)), n_cols)


@pytest.mark.parametrize("n", [65, 1000, 4096, 4097])
def test_draw_counts_and_batches(mm_host, n):
    ds = cases.prefix(W.draw_set("long"), n)
    G, S_ = ds["counts"].shape
    Cc = ds["X"].shape[1]
    # One bound, two terms. for_gene_batches sizes the gene table by (C + 1) n doubles per gene: 2 * 8 * (C + 1) * n + 8 bytes
    # hold two of the three genes, so the table is built twice. cells_in_batches sizes the matching's scratch by its slice of
    # 3 n doubles per cell (beyond the LDS path, n = 4097): the same bytes hold 2 (C + 1) / 3 = 3 cells, fewer than the 8 of a
    # gene's row, so a table batch of 16 cells runs in six launches. At C = 2 the two terms are the same number.
    scratch = 2 * 8 * (Cc + 1) * n + 8
    assert _column_batch(scratch, (Cc + 1) * n, G) == 2 < G and _column_batch(scratch, 3 * n, 2 * S_) == 3 < S_
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_moment_match(k_threshold=0.7)
            sone = h.fit.loo_moment_match(k_threshold=0.7, split=True)
            _lib.testing_set("loo_scratch_bytes", scratch)
            try:
                res = h.fit.loo_moment_match(k_threshold=0.7)
                sres = h.fit.loo_moment_match(k_threshold=0.7, split=True)
                plain = h.fit.loo()
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in MM_KEYS:
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    for k in SPLIT_KEYS:
        assert np.array_equal(sres[k], sone[k], equal_nan=True), k
    assert res["scale"].shape == (G, S_, Cc + 1)
    matched, worst = 0, 0.0
    for g in range(G):
        gene = cases.gene_of(ds, g)
        for s in range(S_):
            ref, _ = R.host_cell(mm_host, gene, s, k_threshold=0.7)
            err = _mm_against(_mm_row(res, g, s), ref, (n, g, s))
            worst = max(worst, err)
            assert err <= _bound("counts"), (n, g, s, err)
            if res["iterations"][g, s] == 0:
                assert all(np.array_equal(res[k][g, s], plain[k][g, s], equal_nan=True) for k in L.FIELDS), (n, g, s)
            matched += res["iterations"][g, s] > 0
    assert np.all(res["scale"][2, :, 1:Cc] == 1.0) and np.all(res["shift"][2, :, 1:Cc] == 0.0)
    print("n", n, "cells matched", int(matched), "largest error against the CPU build", worst)
    assert matched >= 3
    assert worst <= W.WIDE_GPU_MEASURED["counts"]                     # the recorded value is the measured one


def test_moment_matching_plain_and_split(held, mm_host, split_host):
    worst, sworst, matched = 0.0, 0.0, 0
    for c in W.designed():
        ds, fit = W.draw_set(c["set"]), held[c["set"]].fit
        G, S_ = ds["counts"].shape
        Cc = ds["X"].shape[1]
        kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
        re = np.full((1, S_), c["r_eff"])
        res = fit.loo_moment_match([c["g"]], r_eff=re, **kw)
        sres = fit.loo_moment_match([c["g"]], r_eff=re, split=True, **kw)
        plain = fit.loo([c["g"]], r_eff=re)
        assert res["scale"].shape == sres["scale"].shape == (1, S_, Cc + 1) and res["iterations"].dtype == np.int64
        assert sres["khat_split"].shape == (1, S_)
        for k in ("khat", "khat_before", "iterations", "scale", "shift"):            # the split leaves the matching's record alone
            assert np.array_equal(sres[k], res[k], equal_nan=True), (c["name"], k)
        assert np.array_equal(sres["elpd_loo_matched"], res["elpd_loo"], equal_nan=True), c["name"]
        gene = cases.gene_of(ds, c["g"])
        for s in range(S_):                                               # the designed cell and its gene's other cells
            ref, _ = R.host_cell(mm_host, gene, s, r_eff=c["r_eff"], **kw)
            sref = S.host_cell(split_host, gene, s, r_eff=c["r_eff"], **kw)
            err = _mm_against(_mm_row(res, 0, s), ref, (c["name"], s))
            serr = _split_against(_split_row(sres, 0, s), sref, (c["name"], s))
            worst, sworst = max(worst, err), max(sworst, serr)
            assert err <= _bound("mm") and serr <= _bound("split"), (c["name"], s, err, serr)
            if res["iterations"][0, s] == 0:                              # untouched cells: Fit.loo's bits
                for r in (res, sres):
                    assert all(np.array_equal(r[k][0, s], plain[k][0, s], equal_nan=True) for k in L.FIELDS), (c["name"], s)
                assert np.array_equal(res["khat_before"][0, s], plain["khat"][0, s], equal_nan=True)
                assert np.all(res["scale"][0, s] == 1.0) and np.all(res["shift"][0, s] == 0.0) and np.isnan(sres["khat_split"][0, s])
            else:
                assert res["khat"][0, s] < res["khat_before"][0, s] == plain["khat"][0, s]
                matched += 1
        if c["g"] == 2:                                                   # the slopes the gene does not have: exactly 1 and 0
            assert res["iterations"][0, c["s"]] > 0
            assert np.all(res["scale"][0, :, 1:Cc] == 1.0) and np.all(res["shift"][0, :, 1:Cc] == 0.0), c["name"]
        elif c["kinds"]:
            assert np.all(res["shift"][0, c["s"]] != 0.0), c["name"]      # every coordinate of a checked gene moved
    print("wide cells matched", matched, "largest error against the CPU builds: matching", worst, "split", sworst)
    assert matched >= 20
    assert worst <= W.WIDE_GPU_MEASURED["mm"] and sworst <= W.WIDE_GPU_MEASURED["split"]


def test_exact_predictive_under_matching(held, exact_host, split_host):
    """the entry takes checked genes: the designed cells of genes 0 and 1"""
    worst, sworst, matched = 0.0, 0.0, 0
    for c in W.designed():
        if c["g"] >= W.K:
            continue
        ds, fit = W.draw_set(c["set"]), held[c["set"]].fit
        S_, Cc = ds["X"].shape
        kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
        re = np.full((1, S_), c["r_eff"])
        res = fit.loo_predict_exact_moment_match([c["g"]], r_eff=re, truncation_compensation=TC, **kw)
        sres = fit.loo_predict_exact_moment_match([c["g"]], r_eff=re, truncation_compensation=TC, split=True, **kw)
        mm = fit.loo_moment_match([c["g"]], r_eff=re, **kw)
        assert res["scale"].shape == sres["scale"].shape == (1, S_, Cc + 1) and sres["khat_split"].shape == (1, S_)
        for k in ("khat_before", "iterations", "scale", "shift"):         # the matching's own record
            assert np.array_equal(res[k], mm[k], equal_nan=True) and np.array_equal(sres[k], mm[k], equal_nan=True), (c["name"], k)
        gene = cases.gene_of(ds, c["g"])
        for s in range(S_):
            ref = X.host_cell(exact_host, gene, s, r_eff=c["r_eff"], tc=TC, **kw)
            sref = S.host_exact_cell(split_host, gene, s, r_eff=c["r_eff"], tc=TC, **kw)
            err = _exact_against_host(res, 0, s, ref, (c["name"], s))
            serr = _exact_against(sres, 0, s, sref, (c["name"], s))
            worst, sworst = max(worst, err), max(sworst, serr)
            assert err <= _bound("exact") and serr <= _bound("exact_split"), (c["name"], s, err, serr)
            matched += ref[11] > 0
    print("wide cells matched", int(matched), "largest error against the CPU builds: predictive", worst, "split predictive", sworst)
    assert matched >= 16
    assert worst <= W.WIDE_GPU_MEASURED["exact"] and sworst <= W.WIDE_GPU_MEASURED["exact_split"]


@pytest.mark.parametrize("name", SETS)
def test_fit_level_statistics(held, name):
    ds, fit = W.draw_set(name), held[name].fit
    G, S_ = ds["counts"].shape
    n = ds["draws"].shape[0]
    excl = np.isin(np.arange(G * S_), ds["excl"]).reshape(G, S_)
    # ---- Fit.log_lik of every gene against scipy (the slopes unpacked by oracle/independent.py)
    ll = fit.log_lik().reshape(n, G, S_)
    ref, scale = _reference_ll(ds["counts"], ds["X"], ds["expo"], ds["draws"], ds["K"])
    err = np.abs(ll - ref) / scale
    print(name, "largest error of log_lik in units of its terms:", err.max())
    assert err.max() <= 1e-12
    assert np.array_equal(fit.log_lik([2, 0]).reshape(n, 2, S_), ll[:, [2, 0]])
    # ---- Fit.loo of every gene against the restatement on the fit's own log-likelihood
    res = fit.loo()
    ref = L.loo_columns(ll.reshape(n, G * S_), None, excl.ravel())
    assert np.array_equal(res["excluded"], excl)
    for i, k in enumerate(L.FIELDS):
        _compare(res[k].ravel(), ref[:, i], 1e-12, (name, k))
    # ---- the exact predictives of the checked genes, eta in numpy from the fit's columns
    eta, sg = W.columns(ds, lambda idx: fit.columns(idx).reshape(n, len(idx)))
    kw = dict(p_lo=E.P2, p_hi=1 - E.P2, truncation_compensation=E.TC)
    rkw = dict(tc=E.TC, p_lo=E.P2, p_hi=1 - E.P2)
    pe, le = fit.ppc_exact(**kw), fit.loo_predict_exact(**kw)
    assert pe["genes"].tolist() == le["genes"].tolist() == [0, 1] and pe["n_draws"] == n
    used = xused = cells = 0
    for g in range(ds["K"]):
        for s in range(S_):
            y = int(ds["counts"][g, s])
            r = E.point(eta[:, g, s], sg[:, g], y, excluded=bool(excl[g, s]), **rkw)
            used += E.check([float(pe[k][g, s]) for k in E.FIELDS], r, (name, g, s))
            r = XR.point(ll[:, g, s], eta[:, g, s], sg[:, g], y, excluded=bool(excl[g, s]), **rkw)
            xused += XR.check([float(le[k][g, s]) for k in XR.FIELDS], r, (name, g, s))
            cells += 1
    print(name, "cells", cells, "interval ends on the allowance: ppc_exact", used, "loo_predict_exact", xused)
    assert used <= 0.02 * cells and xused <= 0.02 * 2 * cells
    assert np.array_equal(pe["excluded"], excl[:ds["K"]]) and np.array_equal(le["excluded"], excl[:ds["K"]])
    lp = fit.loo_predict(np.arange(ds["K"]), seed=3, **kw)             # k-hat is Fit.loo_predict's, bit for bit
    assert np.array_equal(le["khat"], lp["khat"], equal_nan=True) and np.array_equal(lp["excluded"], excl[:ds["K"]])
    ex = le["excluded"]
    for k in E.FIELDS:                                                    # an excluded cell is the posterior-predictive one
        assert np.array_equal(le[k][ex], pe[k][ex], equal_nan=True), k


def test_subsets_and_permutations_at_four_columns(held):
    fit = held["factor4"].fit
    calls = dict(
        loo=(lambda g: fit.loo(g), L.FIELDS, 3),
        mm=(lambda g: fit.loo_moment_match(g, k_threshold=0.5), MM_KEYS, 3),
        split=(lambda g: fit.loo_moment_match(g, k_threshold=0.5, split=True), SPLIT_KEYS, 3),
        ppc=(lambda g: fit.ppc_exact(g), E.FIELDS, 2),
        exact=(lambda g: fit.loo_predict_exact(g), XR.FIELDS, 2),
        xmm=(lambda g: fit.loo_predict_exact_moment_match(g, k_threshold=0.5, truncation_compensation=TC), XKEYS, 2),
        xsplit=(lambda g: fit.loo_predict_exact_moment_match(g, k_threshold=0.5, truncation_compensation=TC, split=True),
                XKEYS + ("khat_split",), 2))
    for what, (call, keys, ng) in calls.items():
        full, again = call(np.arange(ng)), call(None)
        perm = np.arange(ng)[::-1] if ng == 2 else np.array([1, 2, 0])
        permuted, sub = call(perm), call([ng - 1])
        for k in keys:
            assert np.array_equal(again[k], full[k], equal_nan=True), (what, k)
            assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), (what, k)
            assert np.array_equal(sub[k], full[k][[ng - 1]], equal_nan=True), (what, k)
        if what in ("mm", "xmm"):
            assert (full["iterations"] > 0).sum() >= 4, what
