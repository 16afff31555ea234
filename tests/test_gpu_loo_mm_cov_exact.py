"""The exact leave-one-out predictive under the weights of the matching with the covariance step on the device
(Fit.loo_predict_exact_moment_match_cov; ppcx_fit_loo_predict_exact_moment_match_cov): the checked-gene cells of
tests/loo_mm_cov_exact_cases.py reach the kernel through Model.fit_from_draws and are held to the CPU build of its header
(tests/loo_mm_cov_exact_cpu), split both ways, and to the other device entries of the same call; the draw counts at the
wavefront, the workgroup's stride and the LDS / scratch hand-over on the C = 4 set, with the scratch in batches of two cells
(testing build); the widths 9 and 17 at their own draw counts with the gene table in batches; and a short NUTS fit of the bundled
case: the same bits on every call, for a gene subset and a permuted gene list, r_eff="auto", the refusals, and identify_outliers
with the flag.

Tolerances: integer fields equal, NaN and Inf in the same places; lower / upper may be one count apart only where the
restatement's own F at the count between them is within the bound of p, at most one end in all; khat, khat_before, iterations,
cov_iterations, transform, shift and khat_split bit-equal to Fit.loo_moment_match(cov=True) of the same call; a cell with
iterations == 0 bit-equal to Fit.loo_predict_exact; the reals against the CPU build at ten times the largest error measured (in
units of max(1, |ref|), p_le / p_ge also relatively below 1e-3; X.GPU_MEASURED, the tests print theirs), never above 1e-9."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_cov_cases as cov_cases
from tests import loo_mm_cov_exact_cases as K
from tests import loo_mm_cov_exact_restate as X
from tests import wide_design_cases as W
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_loo_mm import _Held
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

GPU_BOUND = min(10 * X.GPU_MEASURED, X.BOUND)
TEN = ("mean", "sd", "p_le", "p_ge", "lower", "upper", "y", "excluded", "outside", "khat")
STATE = ("khat", "khat_before", "iterations", "cov_iterations", "transform", "shift")
KEYS = TEN + ("pit_lt", "pit_le") + STATE[1:]
NH = len(X.HEAD)
ALLOWED = []                                          # the interval ends that used the allowance, over the whole module: every test that
                                                      # compares with the CPU build asserts, after its own cells, that there is at most one


@pytest.fixture(scope="module")
def host():
    return X.host_lib()


def _row(res, i, s):
    head = [res[k][i, s] for k in X.HEAD[:13]] + [res["khat_split"][i, s] if "khat_split" in res else np.nan]
    return np.concatenate([head, res["transform"][i, s].ravel(), res["shift"][i, s]]).astype(np.float64)


def _against_host(res, i, s, ref, what, point=None):
    """the device's cell against the CPU build's record: the integers and the places of NaN / Inf equal (an interval end one
    count apart: point() gives the restatement's dict for the allowance); returns the error of the rest"""
    got = _row(res, i, s)
    nan = np.isnan(ref[0])
    for k in ("lower", "upper", "y", "excluded", "outside", "iterations", "cov_iterations"):
        j = X.HEAD.index(k)
        if k in ("lower", "upper") and nan:
            assert got[j] == -1 and np.isnan(ref[j]), (what, k)         # the dict's integer for a NaN interval end
        elif k == "outside" and nan:
            assert got[j] == 0 and np.isnan(ref[j]), (what, k)
        elif k in ("lower", "upper") and got[j] != ref[j]:
            r = point()
            f = X.E.mixture_cdf(int(min(got[j], ref[j])), r["w"], r["mu"], r["phi"])
            assert abs(got[j] - ref[j]) == 1 and abs(f - r["p_lo" if k == "lower" else "p_hi"]) <= GPU_BOUND, (what, k, got[j], ref[j], f)
            ALLOWED.append((what, k))
        elif k == "outside" and any(w == what for w, _ in ALLOWED):
            continue
        else:
            assert got[j] == ref[j], (what, k, got[j], ref[j])
    real = [j for j in range(len(ref)) if j >= NH or X.HEAD[j] in X.REALS]
    assert np.array_equal(np.isnan(got[real]), np.isnan(ref[real])) and np.array_equal(np.isinf(got[real]), np.isinf(ref[real])), (what, got, ref)
    return X.errors(got, X.row_dict(ref, res["shift"].shape[-1] - 1))


def _relations(res, cov, diag, plain, split, what):
    """the entry against the other device entries of the same call: the matching's record bit-equal to
    Fit.loo_moment_match(cov=True) (`cov`, with the same split), cells with cov_iterations == 0 within the bound of
    Fit.loo_predict_exact_moment_match (`diag`, with the same split), cells with iterations == 0 bit-equal to
    Fit.loo_predict_exact (`plain`), and p_le + p_ge - 1 = exp(elpd_loo) of the covariance entry. Returns the cells compared
    with `diag`."""
    nc = res["shift"].shape[-1]
    failed = np.isnan(res["mean"]) & (res["iterations"] > 0)             # the predictive failed: khat (and khat_split) go with it
    for k in STATE:
        a, b = res[k], cov[k]
        if k == "khat":
            a, b = a[~failed], b[~failed]
        assert np.array_equal(a, b, equal_nan=True), (what, k)
    assert ("khat_split" in res) == split and "scale" not in res
    if split:
        assert np.array_equal(res["khat_split"][~failed], cov["khat_split"][~failed], equal_nan=True), what
        assert np.all(np.isnan(res["khat_split"][res["iterations"] == 0]))
    it0 = res["iterations"] == 0
    for k in TEN + ("pit_lt", "pit_le"):
        assert np.array_equal(res[k][it0], plain[k][it0], equal_nan=True), (what, k)
    with np.errstate(invalid="ignore"):
        d = np.abs(res["p_le"] + res["p_ge"] - 1.0 - np.exp(cov["elpd_loo"]))
    assert np.array_equal(np.isnan(d), np.isnan(res["mean"]) | np.isnan(cov["elpd_loo"])), what
    assert not np.any(d > 2 * XR.TAILS_ABS + 1e-12), (what, np.nanmax(d))
    seen = 0
    off = ~np.eye(nc, dtype=bool)
    for i, s in zip(*np.nonzero(res["cov_iterations"] == 0)):
        assert np.all(res["transform"][i, s][off] == 0.0), (what, i, s)
        for k in ("lower", "upper", "y", "excluded", "outside", "iterations"):
            assert res[k][i, s] == diag[k][i, s], (what, k, i, s)
        got = np.concatenate([[res[k][i, s] for k in X.REALS[:6]], np.diag(res["transform"][i, s]), res["shift"][i, s]])
        ref = np.concatenate([[diag[k][i, s] for k in X.REALS[:6]], diag["scale"][i, s], diag["shift"][i, s]])
        if split:
            got, ref = np.append(got, res["khat_split"][i, s]), np.append(ref, diag["khat_split"][i, s])
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, i, s, got, ref)
        err = max(X._err(a, b, j in (2, 3)) for j, (a, b) in enumerate(zip(got, ref)))
        assert err <= GPU_BOUND, (what, i, s, err, got, ref)
        seen += 1
    return seen


def _entries(fit, genes, r_eff, split, **kw):
    """(the entry, the covariance matching, the diagonal predictive, the plain predictive) of the same call"""
    return (fit.loo_predict_exact_moment_match_cov(genes, r_eff=r_eff, split=split, **kw),
            fit.loo_moment_match(genes if genes is not None else np.arange(fit.model.K), r_eff=r_eff, cov=True, split=split, **kw),
            fit.loo_predict_exact_moment_match(genes, r_eff=r_eff, split=split, **kw), fit.loo_predict_exact(genes, r_eff=r_eff))


def test_cells_against_the_cpu_build(host):
    held = {}
    worst, per_width, with_cov, without = 0.0, {}, 0, 0
    try:
        for c in K.CELLS:
            ds = K.draw_set(c["set"])
            if c["set"] not in held:
                held[c["set"]] = _Held(ds)
            fit = held[c["set"]].fit
            S_ = ds["counts"].shape[1]
            nc = ds["X"].shape[1] + 1
            kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
            re = np.full((1, S_), c["r_eff"])
            gene = K.gene_of(c)
            for split in (False, True):
                res, cov, diag, plain = _entries(fit, [c["g"]], re, split, **kw)
                assert res["transform"].shape == (1, S_, nc, nc) and res["shift"].shape == (1, S_, nc)
                assert res["iterations"].dtype == res["cov_iterations"].dtype == np.int64 and res["k_threshold"] == c["k_threshold"]
                ref = X.host_cell(host, gene, c["s"], r_eff=c["r_eff"], split=split, **kw)
                assert ref[11] == len(c["kinds"]) and ref[12] == c["kinds"].count(3), (c["name"], ref[:NH])
                err = _against_host(res, 0, c["s"], ref, (c["name"], split),
                                    lambda: X.point(gene, c["s"], r_eff=c["r_eff"], split=split, **kw))
                print(c["name"], "split", split, "kinds", c["kinds"], "khat", ref[10], "->", ref[9], "khat_split", ref[13], "error", err)
                worst = max(worst, err)
                per_width[nc] = max(per_width.get(nc, 0.0), err)
                assert err <= GPU_BOUND, (c["name"], split, err)
                without += _relations(res, cov, diag, plain, split, (c["name"], split))
            with_cov += 3 in c["kinds"]
    finally:
        for h in held.values():
            h.close()
    print("cells with a covariance step", with_cov, "cells compared with the diagonal predictive", without,
          "largest error against the CPU build:", worst, "per width C + 1:", per_width, "interval ends on the allowance:", ALLOWED)
    assert with_cov == 22 and without >= 200
    assert len(ALLOWED) <= 1, ALLOWED                                 # at most one interval end in all, whichever tests have run
    assert worst <= X.GPU_MEASURED                                    # the recorded value is the measured one


def _counts_case(host, ds, th, scratch, cells, what):
    """split=True over the checked genes of ds, once unbatched and once under the scratch bound: the same bits; `cells` against
    the CPU build, the others against the relations. Returns (the batched result, the largest error)."""
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_predict_exact_moment_match_cov(k_threshold=th, split=True)
            _lib.testing_set("loo_scratch_bytes", scratch)
            try:
                res, cov, diag, plain = _entries(h.fit, None, None, True, k_threshold=th)
                uns = h.fit.loo_predict_exact_moment_match_cov(k_threshold=th)
                ucov = h.fit.loo_moment_match(np.arange(ds["K"]), k_threshold=th, cov=True)
                udiag = h.fit.loo_predict_exact_moment_match(k_threshold=th)
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in KEYS + ("khat_split",):
        assert np.array_equal(res[k], one[k], equal_nan=True), (what, k)   # the same bits however the work is batched
    _relations(res, cov, diag, plain, True, what)
    _relations(uns, ucov, udiag, plain, False, what)
    worst = 0.0
    for g, s in cells:
        gene = cases.gene_of(ds, g)
        ref = X.host_cell(host, gene, s, k_threshold=th, split=True)
        err = _against_host(res, g, s, ref, what + (g, s), lambda: X.point(gene, s, k_threshold=th, split=True))
        print(*what, "gene", g, "cell", s, "iterations", ref[11], "cov_iterations", ref[12], "error", err)
        worst = max(worst, err)
        assert err <= GPU_BOUND, (what, g, s, err)
    return res, worst


COUNTS_THRESHOLD = 0.3                                # tests/test_gpu_loo_mm_cov.py's: the outlier cell takes a covariance step from 257 draws on


@pytest.mark.parametrize("n", [1, 2, 5, 6, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097])
def test_draw_counts(host, n):
    """the ends of the wavefront and of the workgroup's stride, n <= d and d + 1, and the LDS / scratch hand-over on prefixes of
    the C = 4 set, split=True; the scratch bound set so that the scratch path runs in batches of two cells. Cell (0, 5) qualifies
    at every count (tests/test_loo_mm_cov_host.py) and is held to the CPU build; the other cells to the relations."""
    ds = cases.prefix(W.draw_set("long"), n)
    res, worst = _counts_case(host, ds, COUNTS_THRESHOLD, 2 * 8 * 3 * n + 8, ((0, 5),), ("long", n))
    print("n", n, "cells matched", int((res["iterations"] > 0).sum()), "with a covariance step", int((res["cov_iterations"] > 0).sum()),
          "largest error against the CPU build", worst)
    assert res["cov_iterations"][0, 5] >= (1 if n >= 257 else 0)
    if n <= 6:
        assert np.all(res["cov_iterations"] == 0)
    assert len(ALLOWED) <= 1, ALLOWED
    assert worst <= X.GPU_MEASURED


WIDTH_CELLS = dict(columns16=(1, 4), columns8=(0, 6))     # the checked-gene cells that DESIGN 8.16 holds to the CPU build


@pytest.mark.parametrize("name,n", [(name, n) for name in cov_cases.WIDEST_COUNTS for n in cov_cases.WIDEST_COUNTS[name]["ns"]])
def test_widths(host, name, n):
    """d = 17 and d = 9 at n <= d, d + 1, the wavefront and the workgroup's stride, split=True; 8 (C + 1) n + 8 bytes hold one of
    the two checked genes' tables, so the table is built twice and the device records of the second batch start behind the
    first's; the same bits as unbatched"""
    spec = cov_cases.WIDEST_COUNTS[name]
    ds = cases.prefix(W.draw_set(name), n)
    Cc = ds["X"].shape[1]
    res, worst = _counts_case(host, ds, spec["threshold"], 8 * (Cc + 1) * n + 8, (WIDTH_CELLS[name],), (name, n))
    print(name, "n", n, "cells matched", int((res["iterations"] > 0).sum()), "with a covariance step", int((res["cov_iterations"] > 0).sum()),
          "largest error against the CPU build", worst)
    if n <= Cc + 1:
        assert np.all(res["cov_iterations"] == 0)
    assert len(ALLOWED) <= 1, ALLOWED
    assert worst <= X.GPU_MEASURED


EXCL = (0 * 21 + 3, 2 * 21 + 20)                     # the two cells the model holds out


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X_, _, K_ = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X_, expo, K_, excl=np.array(EXCL, np.int32), device=0)
    nuts = m.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    yield dict(m=m, counts=counts, K=K_, nuts=nuts, advi=advi)
    nuts.close()
    advi.close()
    m.close()


def test_nuts_fit(fits):
    """the bundled 53 x 21 case, 3 chains x 150 kept draws, two cells held out, at a threshold of 0.3 so that cells are matched"""
    from ppcseq_amd import _lib
    fit, K_ = fits["nuts"], fits["K"]
    S_ = fits["counts"].shape[1]
    kw = dict(k_threshold=0.3)
    full, cov, diag, plain = _entries(fit, None, None, True, **kw)
    assert full["n_draws"] == 450 and full["genes"].tolist() == list(range(K_)) and full["transform"].shape == (K_, S_, 3, 3)
    seen = _relations(full, cov, diag, plain, True, "nuts")
    it, ci = full["iterations"], full["cov_iterations"]
    print("cells matched", int((it > 0).sum()), "of", it.size, "with a covariance step", int((ci > 0).sum()), "compared with the diagonal "
          "predictive", seen)
    assert (it > 0).sum() >= 1 and np.all(ci <= it) and np.all(np.isfinite(full["mean"]))
    assert np.all(full["khat"][it > 0] < full["khat_before"][it > 0])
    assert np.array_equal(full["excluded"], np.isin(np.arange(K_ * S_), EXCL).reshape(K_, S_))
    # the same bits on a second call, for a gene subset and for a permuted gene list
    again = fit.loo_predict_exact_moment_match_cov(split=True, **kw)
    perm = np.random.default_rng(3).permutation(K_)
    permuted = fit.loo_predict_exact_moment_match_cov(perm, split=True, **kw)
    sub = fit.loo_predict_exact_moment_match_cov([K_ - 1, 0], split=True, **kw)
    for k in KEYS + ("khat_split",):
        assert np.array_equal(again[k], full[k], equal_nan=True), k
        assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), k
        assert np.array_equal(sub[k], full[k][[K_ - 1, 0]], equal_nan=True), k
    # without split: the matching's bits, no khat_split
    uns, ucov, udiag, _ = _entries(fit, None, None, False, **kw)
    _relations(uns, ucov, udiag, plain, False, "nuts, unsplit")
    for k in STATE[1:]:
        assert np.array_equal(uns[k], full[k], equal_nan=True), k
    # r_eff = "auto": the relative efficiencies of the covariance matching's call
    auto, auto_cov = fit.loo_predict_exact_moment_match_cov(r_eff="auto", **kw), fit.loo_moment_match(np.arange(K_), r_eff="auto", cov=True, **kw)
    assert auto["r_eff"].shape == (K_, S_) and np.array_equal(auto["r_eff"], auto_cov["r_eff"])
    for k in STATE:
        assert np.array_equal(auto[k], auto_cov[k], equal_nan=True), k
    assert "r_eff" not in full
    # refusals
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_predict_exact_moment_match_cov needs the draws of a NUTS fit.*ADVI fit"):
        fits["advi"].loo_predict_exact_moment_match_cov()
    with pytest.raises(_lib.PpcxError):
        fit.loo_predict_exact_moment_match_cov([K_])                  # not a checked gene
    with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
        fit.loo_predict_exact_moment_match_cov([0], k_threshold=np.nan)
    with pytest.raises(_lib.PpcxError, match="max_iters must be >= 0"):
        fit.loo_predict_exact_moment_match_cov([0], max_iters=-1, split=True)
    with pytest.raises(_lib.PpcxError):
        fit.loo_predict_exact_moment_match_cov([0], p_lo=0.9, p_hi=0.1)


def test_unchecked_genes_of_the_designed_lists_are_refused():
    from ppcseq_amd import _lib
    held = {}
    try:
        for c in K.UNCHECKED:
            if c["set"] not in held:
                held[c["set"]] = _Held(K.draw_set(c["set"]))
            with pytest.raises(_lib.PpcxError):
                held[c["set"]].fit.loo_predict_exact_moment_match_cov([c["g"]])
    finally:
        for h in held.values():
            h.close()
    assert len(K.UNCHECKED) == 5


def test_identify_outliers_with_the_flag(bundled):
    """a short NUTS run of the bundled 53 x 21 case: flags and frame are those of the call without the flag, the attrs carry
    transform and cov_iterations; how many cells took a covariance step is printed, not asserted"""
    import warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11,
              adj_prob_theshold_2=0.01,                     # 1 000 draws in the second pass too: the test stays short
              exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_split=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = identify_outliers(df, **kw)
        out = identify_outliers(df, exact_loo_moment_match_cov=True, **kw)
    assert set(out.attrs) == set(plain.attrs)
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    for key in ("exact_loo_intervals_discovery", "exact_loo_intervals_test"):
        r, p = out.attrs[key], plain.attrs[key]
        assert "transform" in r and "scale" not in r and "cov_iterations" in r and "cov_iterations" not in p and "khat_split" in r, key
        assert r["transform"].shape == (3, 21, 3, 3) and np.array_equal(r["khat_before"], p["khat_before"], equal_nan=True), key
        none = r["cov_iterations"] == 0
        assert np.array_equal(r["iterations"][none], p["iterations"][none]), key
        print(key, "draws", r["n_draws"], "cells matched", int((r["iterations"] > 0).sum()), "with a covariance step", int((~none).sum()))
    with pytest.raises(ValueError, match="^exact_loo_moment_match_cov needs exact_loo_moment_match"):
        identify_outliers(df, **dict(kw, exact_loo_moment_match=False, exact_loo_moment_match_split=False, exact_loo_moment_match_cov=True))
