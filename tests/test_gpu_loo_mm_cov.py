"""Gene-local moment matching with the covariance step on the device (Fit.loo_moment_match(cov=True);
ppcx_fit_loo_moment_match_cov): the designed cells of tests/loo_mm_cov_cases.py reach the kernel through Model.fit_from_draws and
are held to the CPU build of its header (tests/loo_mm_cov_twin), split both ways; the draw counts at the wavefront, the
workgroup's stride and the LDS / scratch hand-over on the C = 4 set, with the scratch in batches of two cells (testing build);
the cells without a covariance step against Fit.loo_moment_match(cov=False) of the same call and the unmatched ones against
Fit.loo; and a short NUTS fit of the bundled case: the same bits on every call, for a gene subset and a permuted gene list,
r_eff="auto", the refusals, and identify_outliers with the flag.

Tolerances: iterations and cov_iterations equal, NaN and Inf in the same places; a cell with iterations == 0 bit-equal to
Fit.loo; the reals against the CPU build at ten times the largest error measured on the designed cells and the draw counts in
units of max(1, |ref|) (V.GPU_MEASURED; the tests print theirs), never above 1e-9."""
import numpy as np
import pytest

from tests import loo_mm_cases as cases
from tests import loo_mm_cov_cases as cov_cases
from tests import loo_mm_cov_restate as V
from tests import loo_restate as L
from tests import wide_design_cases as W
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_loo_mm import _Held
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

GPU_BOUND = min(10 * V.GPU_MEASURED, V.BOUND)
KEYS = V.HEAD[:7] + ("transform", "shift")
SPLIT_KEYS = V.HEAD + ("transform", "shift")


@pytest.fixture(scope="module")
def host():
    return V.host_lib()


def _row(res, i, s):
    """the cell as the header's record; without split the dict has no elpd_loo_matched / khat_split: elpd_loo and NaN"""
    head = [res[k][i, s] for k in V.HEAD[:7]] + [res.get("elpd_loo_matched", res["elpd_loo"])[i, s],
                                                   res["khat_split"][i, s] if "khat_split" in res else np.nan]
    return np.concatenate([head, res["transform"][i, s].ravel(), res["shift"][i, s]]).astype(np.float64)


def _against_host(got, ref, what):
    assert all(got[j] == ref[j] for j in V.INTS), (what, got[:9], ref[:9])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, got, ref)
    return V.errors(got, ref)


def _against_plain_matching(res, un, plain, what):
    """cells with cov_iterations == 0 against Fit.loo_moment_match(cov=False) of the same call (`un`): integers equal, the
    transform diagonal with the scales on it, the reals within the bound; cells with iterations == 0 against Fit.loo bit for bit"""
    nc = res["shift"].shape[-1]
    off = ~np.eye(nc, dtype=bool)
    seen = 0
    for i, s in zip(*np.nonzero(res["cov_iterations"] == 0)):
        assert res["iterations"][i, s] == un["iterations"][i, s], (what, i, s)
        assert np.all(res["transform"][i, s][off] == 0.0), (what, i, s)
        got = np.concatenate([[res[k][i, s] for k in ("elpd_loo", "khat", "khat_before")], np.diag(res["transform"][i, s]), res["shift"][i, s]])
        ref = np.concatenate([[un[k][i, s] for k in ("elpd_loo", "khat", "khat_before")], un["scale"][i, s], un["shift"][i, s]])
        if "khat_split" in res:
            got, ref = np.append(got, [res["khat_split"][i, s], res["elpd_loo_matched"][i, s]]), np.append(ref, [un["khat_split"][i, s], un["elpd_loo_matched"][i, s]])
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, i, s, got, ref)
        assert max(V._err(a, b) for a, b in zip(got, ref)) <= GPU_BOUND, (what, i, s, got, ref)
        seen += 1
    it0 = res["iterations"] == 0
    for k in L.FIELDS:
        assert np.array_equal(res[k][it0], plain[k][it0], equal_nan=True), (what, k)
    assert np.array_equal(res["khat_before"][it0], plain["khat"][it0], equal_nan=True), what
    assert np.all(res["transform"][it0] == np.eye(nc)) and np.all(res["shift"][it0] == 0.0), what
    return seen


def test_designed_cells_against_the_cpu_build(host):
    held = {}
    worst, with_cov, without = 0.0, 0, 0
    try:
        for c in cov_cases.designed():
            ds = cov_cases.draw_set(c["set"])
            if c["set"] not in held:
                held[c["set"]] = _Held(ds)
            fit = held[c["set"]].fit
            S_ = ds["counts"].shape[1]
            nc = ds["X"].shape[1] + 1
            kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
            re = np.full((1, S_), c["r_eff"])
            plain = fit.loo([c["g"]], r_eff=re)
            gene = cov_cases.gene_of(c)
            for split in (False, True):
                res = fit.loo_moment_match([c["g"]], r_eff=re, cov=True, split=split, **kw)
                un = fit.loo_moment_match([c["g"]], r_eff=re, split=split, **kw)
                assert "scale" not in res and res["transform"].shape == (1, S_, nc, nc) and res["shift"].shape == (1, S_, nc)
                assert res["cov_iterations"].dtype == np.int64 and res["k_threshold"] == c["k_threshold"]
                assert ("khat_split" in res) == split and ("elpd_loo_matched" in res) == split
                ref, kinds, _ = V.host_cell(host, gene, c["s"], r_eff=c["r_eff"], split=split, **kw)
                assert kinds == c["kinds"], (c["name"], kinds)
                err = _against_host(_row(res, 0, c["s"]), ref, (c["name"], split))
                print(c["name"], "split", split, "kinds", kinds, "khat", ref[4], "->", ref[3], "error", err)
                worst = max(worst, err)
                assert err <= GPU_BOUND, (c["name"], split, err)
                without += _against_plain_matching(res, un, plain, (c["name"], split))
            with_cov += 3 in c["kinds"]
    finally:
        for h in held.values():
            h.close()
    print("designed cells with a covariance step", with_cov, "cells compared with the plain matching", without,
          "largest error against the CPU build:", worst)
    assert with_cov >= 8 and without >= 40
    assert worst <= V.GPU_MEASURED                                    # the recorded value is the measured one


COUNTS_THRESHOLD = 0.3                                # at it the outlier cell of gene 0 takes a covariance step from 257 draws on
COUNTS_CELLS = ((0, 5), (2, 1))                       # the outlier cell of the checked gene 0 (d = 5), the unchecked gene's (d = 2)


@pytest.mark.parametrize("n", [1, 2, 5, 6, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097])
def test_draw_counts(host, n):
    """the ends of the wavefront and of the workgroup's stride, n <= d and d + 1, and the LDS / scratch hand-over on prefixes of
    the C = 4 set; the scratch bound set so that the scratch path runs in batches of two cells. The two cells held to the CPU
    build qualify at every count (tests/test_loo_mm_cov_host.py); the other cells of the call, whose long runs of marginal
    shifts do not, are held to what needs no reference: the same bits however the work is batched, the plain matching where no
    covariance step was taken, Fit.loo where nothing was matched."""
    ds = cases.prefix(W.draw_set("long"), n)
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_moment_match(k_threshold=COUNTS_THRESHOLD, cov=True, split=True)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)
            try:
                res = h.fit.loo_moment_match(k_threshold=COUNTS_THRESHOLD, cov=True, split=True)
                uns = h.fit.loo_moment_match(k_threshold=COUNTS_THRESHOLD, cov=True)
                un = h.fit.loo_moment_match(k_threshold=COUNTS_THRESHOLD, split=True)
                plain = h.fit.loo()
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in SPLIT_KEYS:
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    for k in KEYS[3:]:
        assert np.array_equal(res[k], uns[k], equal_nan=True), k       # the split leaves the matching's bits alone
    assert np.array_equal(res["elpd_loo_matched"], uns["elpd_loo"], equal_nan=True)
    _against_plain_matching(res, un, plain, n)
    assert np.all(res["transform"][2][:, 1:4, :] == np.eye(5)[1:4]) and np.all(res["transform"][2][:, :, 1:4] == np.eye(5)[:, 1:4])
    assert np.all(res["shift"][2][:, 1:4] == 0.0)                      # the identity rows and columns of the unchecked gene
    worst = 0.0
    for g, s in COUNTS_CELLS:
        ref, kinds, _ = V.host_cell(host, cases.gene_of(ds, g), s, k_threshold=COUNTS_THRESHOLD, split=True)
        err = _against_host(_row(res, g, s), ref, (n, g, s))
        print("n", n, "gene", g, "cell", s, "kinds", kinds, "error", err)
        worst = max(worst, err)
        assert err <= GPU_BOUND, (n, g, s, kinds, err)
    print("n", n, "cells matched", int((res["iterations"] > 0).sum()), "with a covariance step", int((res["cov_iterations"] > 0).sum()),
          "cov_iterations of the outlier cell", res["cov_iterations"][0, 5], "largest error against the CPU build", worst)
    assert res["cov_iterations"][0, 5] >= (1 if n >= 257 else 0)
    if n <= 6:
        assert np.all(res["cov_iterations"] == 0)
    assert worst <= V.GPU_MEASURED                                    # the recorded value is the measured one


EXCL = (0 * 21 + 3, 2 * 21 + 20)                     # the two cells the model holds out


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X_, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X_, expo, K, excl=np.array(EXCL, np.int32), device=0)
    nuts = m.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    yield dict(m=m, counts=counts, K=K, nuts=nuts, advi=advi)
    nuts.close()
    advi.close()
    m.close()


def test_nuts_fit(fits):
    """the bundled 53 x 21 case, 3 chains x 150 kept draws, two cells held out, at a threshold of 0.3 so that cells are matched"""
    from ppcseq_amd import _lib
    fit, K = fits["nuts"], fits["K"]
    G, S_ = fits["counts"].shape
    kw = dict(k_threshold=0.3, cov=True, split=True)
    full, plain = fit.loo_moment_match(**kw), fit.loo()
    un = fit.loo_moment_match(k_threshold=0.3, split=True)
    assert full["n_draws"] == 450 and full["transform"].shape == (G, S_, 3, 3) and "scale" not in full
    seen = _against_plain_matching(full, un, plain, "nuts")
    it, ci = full["iterations"], full["cov_iterations"]
    print("cells matched", int((it > 0).sum()), "of", it.size, "with a covariance step", int((ci > 0).sum()), "compared with the plain "
          "matching", seen, "estimates", full["estimates"]["elpd_loo"], "plain matching", un["estimates"]["elpd_loo"])
    assert (it > 0).sum() >= 1 and np.all(ci <= it) and np.all(np.isfinite(full["elpd_loo"]))
    assert np.all(np.isnan(full["khat_split"][it == 0])) and np.all(np.isfinite(full["khat_split"][it > 0]))
    assert np.all(full["khat"][it > 0] < full["khat_before"][it > 0])
    # the same bits on a second call, for a gene subset and for a permuted gene list
    again = fit.loo_moment_match(**kw)
    perm = np.random.default_rng(3).permutation(G)
    permuted, sub = fit.loo_moment_match(perm, **kw), fit.loo_moment_match([40, 7, 0], **kw)
    for k in SPLIT_KEYS:
        assert np.array_equal(again[k], full[k], equal_nan=True), k
        assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), k
        assert np.array_equal(sub[k], full[k][[40, 7, 0]], equal_nan=True), k
    # without split: the matching's bits, no split keys
    uns = fit.loo_moment_match(k_threshold=0.3, cov=True)
    assert "khat_split" not in uns and "elpd_loo_matched" not in uns
    for k in KEYS[3:]:
        assert np.array_equal(uns[k], full[k], equal_nan=True), k
    assert np.array_equal(uns["elpd_loo"], full["elpd_loo_matched"], equal_nan=True)
    # r_eff = "auto": the relative efficiencies of the plain matching's call
    auto, auto_un = fit.loo_moment_match(np.arange(K), r_eff="auto", **kw), fit.loo_moment_match(np.arange(K), r_eff="auto", k_threshold=0.3)
    assert auto["r_eff"].shape == (K, S_) and np.array_equal(auto["r_eff"], auto_un["r_eff"])
    assert np.array_equal(auto["khat_before"], auto_un["khat_before"], equal_nan=True)
    # cov=False is the method without the keyword, bit for bit and key for key
    off, ref = fit.loo_moment_match(k_threshold=0.3, cov=False), fit.loo_moment_match(k_threshold=0.3)
    assert list(off) == list(ref) and "transform" not in off
    for k in ref:
        if isinstance(ref[k], np.ndarray):
            assert np.array_equal(off[k], ref[k], equal_nan=True), k
    # refusals
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_moment_match_cov needs the draws of a NUTS fit.*ADVI fit"):
        fits["advi"].loo_moment_match(cov=True)
    with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
        fit.loo_moment_match([0], k_threshold=np.nan, cov=True)
    with pytest.raises(_lib.PpcxError, match="max_iters must be >= 0"):
        fit.loo_moment_match([0], max_iters=-1, cov=True, split=True)


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
              check_loo=True, loo_moment_match=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = identify_outliers(df, **kw)
        out = identify_outliers(df, loo_moment_match_cov=True, **kw)
    assert set(out.attrs) == set(plain.attrs)
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    for key in ("loo_discovery", "loo_test"):
        r, p = out.attrs[key], plain.attrs[key]
        assert "transform" in r and "scale" not in r and "cov_iterations" in r and "cov_iterations" not in p, key
        assert r["transform"].shape == (3, 21, 3, 3) and np.array_equal(r["khat_before"], p["khat_before"], equal_nan=True), key
        none = r["cov_iterations"] == 0
        assert np.array_equal(r["iterations"][none], p["iterations"][none]), key
        print(key, "draws", r["n_draws"], "cells matched", int((r["iterations"] > 0).sum()), "with a covariance step", int((~none).sum()))
    with pytest.raises(ValueError, match="^loo_moment_match_cov needs loo_moment_match"):
        identify_outliers(df, **dict(kw, loo_moment_match=False, loo_moment_match_cov=True))
