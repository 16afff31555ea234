"""The per-cell statistics at the widest designs the library takes, on the device: C = 8 with a continuous covariate, C = 16 (kMaxC)
and the 16-column set cut down to 15 columns ((C + 1)^2 = 256 = the workgroup's size), the draw sets "columns8", "columns16" and
"columns15" of tests/wide_design_cases.py, through Model.fit_from_draws. Fit.loo_moment_match (plain, split, cov, cov and split)
and Fit.loo_predict_exact_moment_match (plain, split) are held to the CPU builds of their headers on the designed cells of
wide_design_cases.designed(widest=True) and loo_mm_cov_cases.designed(widest=True); the draw counts of the covariance kernel
(n <= d, the wavefront, the workgroup's stride); every entry with the gene table in batches; Fit.log_lik, Fit.loo, Fit.ppc_exact
and Fit.loo_predict_exact against scipy and their restatements; gene subsets and permuted gene lists; and the refusal of a
continuous covariate among nine columns.

Tolerances: iterations, cov_iterations and the other integer fields equal, NaN and Inf in the same places, a cell with
iterations == 0 bit-equal to Fit.loo; the reals against the CPU builds at ten times the largest error measured on these cells in
units of max(1, |ref|) (W.WIDEST_GPU_MEASURED, one value per statistic and width; each test prints its own), never above 1e-9.
`diag`: cells on whose path no covariance step was accepted, cov=True against cov=False of the same call. The fit-level
statistics: the tolerances of tests/test_gpu_loo.py, tests/test_gpu_ppc_exact.py and tests/test_gpu_loo_exact.py.
tests/test_widest_designs_host.py holds the CPU builds to the restatements on the same cells and asserts that every one qualifies."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_cov_cases as cov_cases
from tests import loo_mm_cov_restate as V
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as S
from tests import loo_restate as L
from tests import ppc_exact_restate as E
from tests import wide_design_cases as W
from tests.gpu_fixtures import testing_library
from tests.test_gpu_loo import _compare, _reference_ll
from tests.test_gpu_loo_mm import _Held, _against_host as _mm_against, _row as _mm_row
from tests.test_gpu_loo_mm_cov import _against_host as _cov_against, _row as _cov_row
from tests.test_gpu_loo_mm_exact import _against_host as _exact_against_host
from tests.test_gpu_loo_mm_split import _against_host as _split_against, _exact_against, _row as _split_row

pytestmark = pytest.mark.gpu

TC = 0.7352941
MM_KEYS = R.HEAD + ("scale", "shift")
SPLIT_KEYS = MM_KEYS + S.TAIL
COV_KEYS = V.HEAD[:7] + ("transform", "shift")
COV_SPLIT_KEYS = V.HEAD + ("transform", "shift")
XKEYS = X.HEAD + ("scale", "shift", "pit_lt", "pit_le")
ALL_SETS = W.WIDEST + ("columns15",)


def _bound(name, what):
    return min(10 * W.WIDEST_GPU_MEASURED[name][what], W.BOUND)


def _check_recorded(worst, what):
    """the recorded values are the measured ones, to the two digits kept"""
    for name, w in worst.items():
        rec = W.WIDEST_GPU_MEASURED[name][what]
        assert w <= rec and rec - w <= 0.1 * rec, (name, what, w, rec)


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
def cov_host():
    return V.host_lib()


@pytest.fixture(scope="module")
def held():
    """the three draw sets as models and fits of the product library"""
    h = {}
    try:
        for name in ALL_SETS:
            h[name] = _Held(W.draw_set(name))
        yield h
    finally:
        for x in h.values():
            x.close()


def _column_batch(scratch_bytes, rows, n_cols):
    """column_batch of ppcx_columns.h: columns of `rows` doubles under the bound, at least one, at most all"""
    return min(max(1, scratch_bytes // (8 * rows)), n_cols)


def _untouched_cells_are_loo(res, plain, what):
    it0 = res["iterations"] == 0
    for k in L.FIELDS:
        assert np.array_equal(res[k][it0], plain[k][it0], equal_nan=True), (what, k)
    assert np.array_equal(res["khat_before"], plain["khat"], equal_nan=True), what
    m = ~it0
    assert np.all(res["khat"][m] < res["khat_before"][m]), what


def test_moment_matching_plain_and_split(held, mm_host, split_host):
    worst, sworst, matched = dict.fromkeys(W.WIDEST, 0.0), dict.fromkeys(W.WIDEST, 0.0), 0
    for c in W.designed(widest=True):
        ds, fit = W.draw_set(c["set"]), held[c["set"]].fit
        S_, Cc = ds["X"].shape
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
        ref, kinds = R.host_cell(mm_host, gene, c["s"], r_eff=c["r_eff"], **kw)
        sref = S.host_cell(split_host, gene, c["s"], r_eff=c["r_eff"], **kw)
        assert kinds == c["kinds"], (c["name"], kinds)
        err = _mm_against(_mm_row(res, 0, c["s"]), ref, c["name"])
        serr = _split_against(_split_row(sres, 0, c["s"]), sref, c["name"])
        print(c["name"], "kinds", kinds, "error: matching", err, "split", serr)
        worst[c["set"]], sworst[c["set"]] = max(worst[c["set"]], err), max(sworst[c["set"]], serr)
        assert err <= _bound(c["set"], "mm") and serr <= _bound(c["set"], "split"), (c["name"], err, serr)
        for r in (res, sres):                                             # the gene's other cells: what needs no reference
            _untouched_cells_are_loo(r, plain, c["name"])
        it0 = res["iterations"] == 0
        assert np.all(res["scale"][it0] == 1.0) and np.all(res["shift"][it0] == 0.0) and np.all(np.isnan(sres["khat_split"][it0]))
        matched += int((~it0).sum())
        if c["g"] == 2:                                                   # the slopes the gene does not have: exactly 1 and 0
            assert res["iterations"][0, c["s"]] > 0
            assert np.all(res["scale"][0, :, 1:Cc] == 1.0) and np.all(res["shift"][0, :, 1:Cc] == 0.0), c["name"]
        elif c["kinds"]:
            assert np.all(res["shift"][0, c["s"]] != 0.0), c["name"]      # every coordinate of a checked gene moved
    print("widest cells matched", matched, "largest error against the CPU builds: matching", worst, "split", sworst)
    assert matched >= 40
    _check_recorded(worst, "mm")
    _check_recorded(sworst, "split")


def test_exact_predictive_under_matching(held, exact_host, split_host):
    """the entry takes checked genes: the designed cells of genes 0 and 1"""
    worst, sworst, matched = dict.fromkeys(W.WIDEST, 0.0), dict.fromkeys(W.WIDEST, 0.0), 0
    for c in W.designed(widest=True):
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
        ref = X.host_cell(exact_host, gene, c["s"], r_eff=c["r_eff"], tc=TC, **kw)
        sref = S.host_exact_cell(split_host, gene, c["s"], r_eff=c["r_eff"], tc=TC, **kw)
        err = _exact_against_host(res, 0, c["s"], ref, c["name"])
        serr = _exact_against(sres, 0, c["s"], sref, c["name"])
        print(c["name"], "error: predictive", err, "split predictive", serr)
        worst[c["set"]], sworst[c["set"]] = max(worst[c["set"]], err), max(sworst[c["set"]], serr)
        assert err <= _bound(c["set"], "exact") and serr <= _bound(c["set"], "exact_split"), (c["name"], err, serr)
        matched += ref[11] > 0
    print("widest cells matched", int(matched), "largest error against the CPU builds: predictive", worst, "split predictive", sworst)
    assert matched >= 14
    _check_recorded(worst, "exact")
    _check_recorded(sworst, "exact_split")


def _against_plain_matching(res, un, plain, bound, what):
    """tests/test_gpu_loo_mm_cov.py's comparison with the bound of these widths: cells with cov_iterations == 0 against
    Fit.loo_moment_match(cov=False) of the same call (`un`): integers equal, the transform diagonal with the scales on it; cells
    with iterations == 0 against Fit.loo bit for bit. Returns (cells compared, their largest error)."""
    nc = res["shift"].shape[-1]
    off = ~np.eye(nc, dtype=bool)
    seen, worst = 0, 0.0
    for i, s in zip(*np.nonzero(res["cov_iterations"] == 0)):
        assert res["iterations"][i, s] == un["iterations"][i, s], (what, i, s)
        assert np.all(res["transform"][i, s][off] == 0.0), (what, i, s)
        got = np.concatenate([[res[k][i, s] for k in ("elpd_loo", "khat", "khat_before")], np.diag(res["transform"][i, s]), res["shift"][i, s]])
        ref = np.concatenate([[un[k][i, s] for k in ("elpd_loo", "khat", "khat_before")], un["scale"][i, s], un["shift"][i, s]])
        if "khat_split" in res:
            got, ref = np.append(got, [res["khat_split"][i, s], res["elpd_loo_matched"][i, s]]), np.append(ref, [un["khat_split"][i, s], un["elpd_loo_matched"][i, s]])
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, i, s, got, ref)
        err = max(V._err(a, b) for a, b in zip(got, ref))
        assert err <= bound, (what, i, s, err, got, ref)
        seen, worst = seen + 1, max(worst, err)
    it0 = res["iterations"] == 0
    for k in L.FIELDS:
        assert np.array_equal(res[k][it0], plain[k][it0], equal_nan=True), (what, k)
    assert np.array_equal(res["khat_before"][it0], plain["khat"][it0], equal_nan=True), what
    assert np.all(res["transform"][it0] == np.eye(nc)) and np.all(res["shift"][it0] == 0.0), what
    return seen, worst


def _unchecked_gene_keeps_the_identity(res, i, Cc, what):
    """rows and columns 1 .. C - 1 of the unchecked gene's transform are the identity's, its shift there 0"""
    eye = np.eye(Cc + 1)
    assert np.all(res["transform"][i][:, 1:Cc, :] == eye[1:Cc]) and np.all(res["transform"][i][:, :, 1:Cc] == eye[:, 1:Cc]), what
    assert np.all(res["shift"][i][:, 1:Cc] == 0.0), what


def test_covariance_form_against_the_cpu_build(held, cov_host):
    """every designed cell of the covariance form, split both ways: the record's shape, the cell against the CPU build, the
    gene's other cells against the plain matching and Fit.loo. The 15-column cells reach (C + 1)^2 = 256 = kBlockThreads, the
    16-column ones the second trip of the workgroup's fill of a matrix."""
    worst, dworst = dict.fromkeys(ALL_SETS, 0.0), dict.fromkeys(ALL_SETS, 0.0)
    with_cov, without = dict.fromkeys((2, 9, 16, 17), 0), 0
    for c in cov_cases.designed(widest=True):
        ds, fit = W.draw_set(c["set"]), held[c["set"]].fit
        S_, Cc = ds["X"].shape
        nc = Cc + 1
        kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
        re = np.full((1, S_), c["r_eff"])
        plain = fit.loo([c["g"]], r_eff=re)
        gene = cases.gene_of(ds, c["g"])
        for split in (False, True):
            res = fit.loo_moment_match([c["g"]], r_eff=re, cov=True, split=split, **kw)
            un = fit.loo_moment_match([c["g"]], r_eff=re, split=split, **kw)
            assert "scale" not in res and res["transform"].shape == (1, S_, nc, nc) and res["shift"].shape == (1, S_, nc)
            assert res["cov_iterations"].dtype == np.int64 and res["k_threshold"] == c["k_threshold"]
            assert ("khat_split" in res) == split and ("elpd_loo_matched" in res) == split
            ref, kinds, _ = V.host_cell(cov_host, gene, c["s"], r_eff=c["r_eff"], split=split, **kw)
            assert kinds == c["kinds"], (c["name"], kinds)
            err = _cov_against(_cov_row(res, 0, c["s"]), ref, (c["name"], split))
            print(c["name"], "split", split, "kinds", kinds, "khat", ref[4], "->", ref[3], "error", err)
            worst[c["set"]] = max(worst[c["set"]], err)
            assert err <= _bound(c["set"], "cov"), (c["name"], split, err)
            seen, derr = _against_plain_matching(res, un, plain, _bound(c["set"], "diag"), (c["name"], split))
            without, dworst[c["set"]] = without + seen, max(dworst[c["set"]], derr)
            assert np.all(np.triu(res["transform"][0], 1) == 0.0), c["name"]     # products of lower triangles and diagonals
            if c["g"] == 2:
                _unchecked_gene_keeps_the_identity(res, 0, Cc, c["name"])
        if 3 in c["kinds"]:
            with_cov[len(V.coords(gene))] += 1
    print("designed cells with a covariance step per d", with_cov, "cells compared with the plain matching", without,
          "largest error against the CPU build:", worst, "of cov=True against cov=False without a covariance step:", dworst)
    assert with_cov[17] >= 2 and with_cov[9] >= 2 and with_cov[16] >= 1 and with_cov[2] >= 1 and without >= 200
    _check_recorded(worst, "cov")
    _check_recorded(dworst, "diag")


@pytest.mark.parametrize("name", W.WIDEST)
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


def _entries(fit, threshold=0.5):
    """every per-cell entry as (call of a gene list, the keys that hold arrays, the genes it takes)"""
    return dict(
        loo=(lambda g: fit.loo(g), L.FIELDS, 3),
        mm=(lambda g: fit.loo_moment_match(g, k_threshold=threshold), MM_KEYS, 3),
        split=(lambda g: fit.loo_moment_match(g, k_threshold=threshold, split=True), SPLIT_KEYS, 3),
        cov=(lambda g: fit.loo_moment_match(g, k_threshold=threshold, cov=True), COV_KEYS, 3),
        cov_split=(lambda g: fit.loo_moment_match(g, k_threshold=threshold, cov=True, split=True), COV_SPLIT_KEYS, 3),
        ppc=(lambda g: fit.ppc_exact(g), E.FIELDS, 2),
        exact=(lambda g: fit.loo_predict_exact(g), XR.FIELDS, 2),
        xmm=(lambda g: fit.loo_predict_exact_moment_match(g, k_threshold=threshold, truncation_compensation=TC), XKEYS, 2),
        xsplit=(lambda g: fit.loo_predict_exact_moment_match(g, k_threshold=threshold, truncation_compensation=TC, split=True),
                XKEYS + ("khat_split",), 2))


@pytest.mark.parametrize("name", W.WIDEST)
def test_subsets_and_permutations(held, name):
    for what, (call, keys, ng) in _entries(held[name].fit).items():
        full, again = call(np.arange(ng)), call(None)
        perm = np.arange(ng)[::-1] if ng == 2 else np.array([1, 2, 0])
        permuted, sub = call(perm), call([ng - 1])
        for k in keys:
            assert np.array_equal(again[k], full[k], equal_nan=True), (name, what, k)
            assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), (name, what, k)
            assert np.array_equal(sub[k], full[k][[ng - 1]], equal_nan=True), (name, what, k)
        if what in ("mm", "xmm", "cov"):
            assert (full["iterations"] > 0).sum() >= 8, (name, what)
        if what == "cov":
            assert (full["cov_iterations"] > 0).sum() >= 4, name


@pytest.mark.parametrize("name", W.WIDEST)
def test_both_walks_in_batches(name):
    """2 * 8 * (C + 1) * n + 8 bytes hold two of the three genes' tables of (C + 1) n doubles, so the table is built twice, and
    2 (C + 1) / 3 of a row's cells' scratch slices: every entry gives the bits of the unbatched call"""
    ds = W.draw_set(name)
    G, S_ = ds["counts"].shape
    Cc, n = ds["X"].shape[1], ds["draws"].shape[0]
    scratch = 2 * 8 * (Cc + 1) * n + 8
    assert _column_batch(scratch, (Cc + 1) * n, G) == 2 < G and _column_batch(scratch, 3 * n, 2 * S_) == 2 * (Cc + 1) // 3 < S_
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = {what: call(None) for what, (call, keys, ng) in _entries(h.fit, 0.3).items()}
            _lib.testing_set("loo_scratch_bytes", scratch)
            try:
                res = {what: call(None) for what, (call, keys, ng) in _entries(h.fit, 0.3).items()}
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
            keys = {what: k for what, (call, k, ng) in _entries(h.fit).items()}
        finally:
            h.close()
    for what in one:
        for k in keys[what]:
            assert np.array_equal(res[what][k], one[what][k], equal_nan=True), (name, what, k)
    print(name, "cells matched", int((one["cov"]["iterations"] > 0).sum()), "with a covariance step", int((one["cov"]["cov_iterations"] > 0).sum()))
    assert (one["cov"]["cov_iterations"] > 0).sum() >= 8


@pytest.mark.parametrize("name,n", [(name, n) for name in cov_cases.WIDEST_COUNTS for n in cov_cases.WIDEST_COUNTS[name]["ns"]])
def test_draw_counts_of_the_covariance_kernel(cov_host, name, n):
    """n <= d and d + 1, the ends of the wavefront and of the workgroup's stride on prefixes of the sets, split=True, the gene
    table in batches. The two cells held to the CPU build qualify at every count (tests/test_widest_designs_host.py); the other
    cells of the call are held to what needs no reference: the same bits batched and unbatched, the plain matching where no
    covariance step was taken, Fit.loo where nothing was matched, the identity rows and columns of the unchecked gene."""
    spec = cov_cases.WIDEST_COUNTS[name]
    th = spec["threshold"]
    ds = cases.prefix(W.draw_set(name), n)
    Cc = ds["X"].shape[1]
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_moment_match(k_threshold=th, cov=True, split=True)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * (Cc + 1) * n + 8)
            try:
                res = h.fit.loo_moment_match(k_threshold=th, cov=True, split=True)
                uns = h.fit.loo_moment_match(k_threshold=th, cov=True)
                un = h.fit.loo_moment_match(k_threshold=th, split=True)
                plain = h.fit.loo()
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in COV_SPLIT_KEYS:
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    for k in COV_KEYS[3:]:
        assert np.array_equal(res[k], uns[k], equal_nan=True), k       # the split leaves the matching's bits alone
    assert np.array_equal(res["elpd_loo_matched"], uns["elpd_loo"], equal_nan=True)
    _against_plain_matching(res, un, plain, _bound(name, "diag"), (name, n))
    _unchecked_gene_keeps_the_identity(res, 2, Cc, (name, n))
    worst = 0.0
    for g, s in spec["cells"]:
        ref, kinds, _ = V.host_cell(cov_host, cases.gene_of(ds, g), s, k_threshold=th, split=True)
        err = _cov_against(_cov_row(res, g, s), ref, (name, n, g, s))
        print(name, "n", n, "gene", g, "cell", s, "kinds", kinds, "error", err)
        worst = max(worst, err)
        assert err <= _bound(name, "counts"), (name, n, g, s, kinds, err)
        if (g, s) == spec["cells"][0]:
            assert res["cov_iterations"][g, s] == kinds.count(3) and (3 in kinds or n < 255)     # the CPU build says so from 255 on
    ci = res["cov_iterations"]
    print(name, "n", n, "cells matched", int((res["iterations"] > 0).sum()), "with a covariance step", int((ci > 0).sum()),
          "still above the threshold (candidate 3 reached)", int((res["khat"] > th).sum()), "largest error against the CPU build", worst)
    if n <= Cc + 1:                                                       # n <= d of a checked gene: the refusal, and it was met
        assert np.all(ci == 0) and (res["khat"][:W.K] > th).any()
    assert worst <= W.WIDEST_GPU_MEASURED[name]["counts"]             # the recorded value covers every count


def test_a_continuous_covariate_among_nine_columns_is_still_refused():
    from ppcseq_amd import _lib
    ds = W.draw_set("columns8")
    X9 = np.hstack([ds["X"], np.zeros((ds["X"].shape[0], 1))])
    X9[8, 8] = 1.0                                                        # a ninth column, an indicator: the covariate stays
    with pytest.raises(_lib.PpcxError, match="ppcx error -6: more than 8 design columns are supported for designs of a column of ones "
                                             "and 0 / 1 indicator columns only"):
        _lib.Model(ds["counts"], X9, ds["expo"], ds["K"], lambda_mu_mu=ds["lambda_mu_mu"], device=0)
    X9[:, 7] = (np.arange(X9.shape[0]) == 7).astype(np.float64)           # with the covariate an indicator the design is taken
    _lib.Model(ds["counts"], X9, ds["expo"], ds["K"], lambda_mu_mu=ds["lambda_mu_mu"], device=0).close()
