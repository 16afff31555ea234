"""Gene-local moment matching of the PSIS-LOO cells of an ADVI fit on the device (Fit.loo_moment_match_approximate_posterior,
ppcx_fit_loo_moment_match_approx) and the exact predictive under its weights
(Fit.loo_predict_exact_moment_match_approximate_posterior, ppcx_fit_loo_predict_exact_moment_match_approx): the designed draws and
log ratios of tests/loo_mm_ap_cases.py reach the kernels through the testing build's fit over host-given draws and log ratios
(Model.testing_fit_from_draws_approx) and are held to the CPU build of their header (tests/loo_mm_ap_cpu); the draw counts at the
wavefront, at the workgroup's stride and at the LDS / scratch hand-over, with the scratch in batches of two cells; a short real
ADVI fit of the bundled 53 x 21 case with two excluded cells; and identify_outliers with each modifier.

The predictive entry takes checked genes only, and gene 1 of the tiny model is not one: test_gpu_loo_mm_exact.checked_all gives it
a slope column, so that both genes can be asked for; the CPU build reads the same gene, and a is the array it was.

Tolerances: iterations equal, NaN and Inf in the same places, the cells with iterations = 0 bit-equal to
Fit.loo_approximate_posterior / Fit.loo_predict_exact_approximate_posterior; the other fields against the CPU build at ten times
the largest error measured on the designed cells and the draw counts in units of max(1, |ref|), p_le / p_ge also relatively
below 1e-3 (A.GPU_MEASURED; test_designed_cells_against_the_cpu_build and test_draw_counts print theirs), never above 1e-9."""
import warnings

import numpy as np
import pytest

from tests import loo_mm_ap_cases as cases
from tests import loo_mm_ap_restate as A
from tests import loo_mm_cases as M
from tests import loo_mm_exact_restate as E
from tests import loo_mm_restate as R
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_loo_mm_exact import _against_host as _exact_against_host, checked_all
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

GPU_BOUND = min(10 * A.GPU_MEASURED, A.BOUND)
TC = 0.7352941
LOO4 = ("elpd_loo", "p_loo", "looic", "khat")
MM_KEYS = ("khat", "khat_before", "iterations", "scale", "shift")
KEYS = R.HEAD + ("scale", "shift")
TEN = ("mean", "sd", "p_le", "p_ge", "lower", "upper", "y", "excluded", "outside", "khat")
XKEYS = TEN + ("pit_lt", "pit_le") + MM_KEYS[1:]


@pytest.fixture(scope="module")
def host():
    return A.host_lib()


class _Held:
    """a draw set as a model and a fit over its draws and log ratios (inside testing_library())"""

    def __init__(self, _lib, ds):
        self.m = _lib.Model(ds["counts"], ds["X"], ds["expo"], ds["K"], lambda_mu_mu=ds["lambda_mu_mu"],
                            excl=np.asarray(ds["excl"], np.int32), device=0)
        self.fit = self.m.testing_fit_from_draws_approx(ds["draws"], ds["a"])

    def close(self):
        self.fit.close()
        self.m.close()


def _row(res, i, s):
    return np.concatenate([[res[k][i, s] for k in R.HEAD], res["scale"][i, s], res["shift"][i, s]]).astype(np.float64)


def _against_host(got, ref, what):
    assert got[5] == ref[5], (what, got[5], ref[5])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, got, ref)
    return R.errors(got, ref)


def _untouched(res, plain, xres, xplain, what):
    """cells with iterations == 0 hold the plain approximate-posterior entries' bits; the two forms agree on the matching's record"""
    it0 = res["iterations"] == 0
    for k in LOO4:
        assert np.array_equal(res[k][it0], plain[k][it0], equal_nan=True), (what, k)
    assert np.array_equal(res["khat_before"], plain["khat"], equal_nan=True), what
    assert np.all(res["scale"][it0] == 1.0) and np.all(res["shift"][it0] == 0.0), what
    xit0 = xres["iterations"] == 0
    for k in TEN + ("pit_lt", "pit_le"):
        assert np.array_equal(xres[k][xit0], xplain[k][xit0], equal_nan=True), (what, k)
    assert np.array_equal(xres["khat_before"], xplain["khat"], equal_nan=True), what


def test_designed_cells_against_the_cpu_build(host):
    worst, worst_x, matched = 0.0, 0.0, 0
    with testing_library() as _lib:
        held, sets = {}, {}
        try:
            for c in cases.designed():
                if c["set"] not in held:
                    ds = cases.draw_set(c["set"])
                    sets[c["set"]] = (ds, checked_all(ds))
                    held[c["set"]] = (_Held(_lib, ds), _Held(_lib, sets[c["set"]][1]))
                (ds, xds), (h, xh) = sets[c["set"]], held[c["set"]]
                S = ds["counts"].shape[1]
                kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
                res, plain = h.fit.loo_moment_match_approximate_posterior([c["g"]], **kw), h.fit.loo_approximate_posterior([c["g"]])
                xres = xh.fit.loo_predict_exact_moment_match_approximate_posterior([c["g"]], truncation_compensation=TC, **kw)
                xplain = xh.fit.loo_predict_exact_approximate_posterior([c["g"]], truncation_compensation=TC)
                assert res["k_threshold"] == c["k_threshold"] and res["iterations"].dtype == np.int64 and res["scale"].shape == (1, S, 3)
                assert res["khat_approximation"] == h.fit.psis(cols=[], overall=True)["khat"][-1] or np.isnan(res["khat_approximation"])
                _untouched(res, plain, xres, xplain, c["name"])
                gene, xgene = M.gene_of(ds, c["g"]), M.gene_of(xds, c["g"])
                for s in range(S):                                        # the designed cell and its gene's other cells
                    ref, _ = A.host_cell(host, gene, ds["a"], s, **kw)
                    err = _against_host(_row(res, 0, s), ref, (c["name"], s))
                    xref = A.host_exact_cell(host, xgene, xds["a"], s, tc=TC, **kw)
                    xerr = _exact_against_host(xres, 0, s, xref, (c["name"], s, "predictive"))
                    worst, worst_x = max(worst, err), max(worst_x, xerr)
                    assert err <= GPU_BOUND and xerr <= GPU_BOUND, (c["name"], s, err, xerr)
                    matched += ref[5] > 0
                    if bool(gene["excl"][s]) and not np.isnan(ref[3]):
                        assert res["khat"][0, s] == res["khat_approximation"]    # an excluded cell's khat is the overall one
        finally:
            for pair in held.values():
                for h in pair:
                    h.close()
    print("cells matched", int(matched), "largest error against the CPU build: the elpd form", worst, "the predictive form", worst_x)
    assert matched >= 12
    assert max(worst, worst_x) <= A.GPU_MEASURED                      # the recorded value is the measured one


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 4096, 4097])
def test_draw_counts(host, n):
    """the wavefront, the workgroup's stride (kBlockThreads = 256) and the LDS / scratch hand-over (kPsisLdsDraws = 4 096); the
    scratch bound set so that the scratch path runs in batches of two cells (and the gene table in batches of two genes)"""
    ds = cases.prefix(cases.long_set(), n)
    xds = checked_all(ds)
    with testing_library() as _lib:
        h, xh = _Held(_lib, ds), _Held(_lib, xds)
        try:
            one = h.fit.loo_moment_match_approximate_posterior(k_threshold=0.7)
            xone = xh.fit.loo_predict_exact_moment_match_approximate_posterior(k_threshold=0.7)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)
            try:
                res, plain = h.fit.loo_moment_match_approximate_posterior(k_threshold=0.7), h.fit.loo_approximate_posterior()
                xres = xh.fit.loo_predict_exact_moment_match_approximate_posterior(k_threshold=0.7)
                xmm, xplain = xh.fit.loo_moment_match_approximate_posterior(k_threshold=0.7), xh.fit.loo_predict_exact_approximate_posterior()
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
            xh.close()
    for k in KEYS:
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    for k in XKEYS:
        assert np.array_equal(xres[k], xone[k], equal_nan=True), k
    for k in MM_KEYS:
        assert np.array_equal(xres[k], xmm[k], equal_nan=True), k      # the matching's own record
    _untouched(res, plain, xres, xplain, n)
    matched, worst, where = 0, 0.0, None
    for g in range(2):
        gene, xgene = M.gene_of(ds, g), M.gene_of(xds, g)
        for s in range(4):
            ref, _ = A.host_cell(host, gene, ds["a"], s, k_threshold=0.7)
            err = _against_host(_row(res, g, s), ref, (n, g, s))
            xerr = _exact_against_host(xres, g, s, A.host_exact_cell(host, xgene, xds["a"], s, k_threshold=0.7), (n, g, s, "predictive"))
            if max(err, xerr) > worst:
                worst, where = max(err, xerr), (g, s, "elpd" if err >= xerr else "predictive", int(ref[5]), ref[4], ref[3])
            assert err <= GPU_BOUND and xerr <= GPU_BOUND, (n, g, s, err, xerr)
            matched += res["iterations"][g, s] > 0
    print("n", n, "cells matched", int(matched), "largest error against the CPU build", worst,
          "at (gene, sample, form, iterations, khat_before, khat)", where)
    assert matched >= 1
    assert worst <= A.GPU_MEASURED


EXCL = (0 * 21 + 3, 2 * 21 + 20)                     # the two cells the model holds out


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X, expo, K, excl=np.array(EXCL, np.int32), device=0)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    yield dict(m=m, counts=counts, K=K, advi=advi)
    advi.close()
    m.close()


def test_advi_fit(fits):
    from ppcseq_amd import _lib
    from ppcseq_amd.inference import loo_threshold
    f, fit, K = fits, fits["advi"], fits["K"]
    G, S = f["counts"].shape
    full, plain = fit.loo_moment_match_approximate_posterior(), fit.loo_approximate_posterior()
    xfull, xplain = fit.loo_predict_exact_moment_match_approximate_posterior(), fit.loo_predict_exact_approximate_posterior()
    thr = full["k_threshold"]
    overall = float(fit.psis(cols=[], overall=True)["khat"][-1])
    assert thr == xfull["k_threshold"] == loo_threshold(300) and full["n_draws"] == 300
    assert full["khat_approximation"] == xfull["khat_approximation"] == overall
    assert full["scale"].shape == (G, S, 3) and xfull["scale"].shape == (K, S, 3) and full["excluded"].sum() == 2
    it = full["iterations"]
    assert it.dtype == np.int64 and np.all(it >= 0) and np.all(it <= 30) and np.all(full["khat_before"][it > 0] > thr)
    assert np.all(full["khat"][it > 0] < full["khat_before"][it > 0])
    assert np.all(full["khat"][full["excluded"]] == overall) and np.all(it[full["excluded"]] == 0)
    assert np.all(full["scale"][K:, :, 1] == 1.0) and np.all(full["shift"][K:, :, 1] == 0.0)    # genes without a slope
    _untouched(full, plain, xfull, xplain, "fit")
    # the two entries agree on the matching's record bit for bit (khat: unless the predictive itself failed)
    for k in MM_KEYS[1:]:
        assert np.array_equal(xfull[k], full[k][:K], equal_nan=True), k
    failed = np.isnan(xfull["mean"])
    assert np.array_equal(xfull["khat"][~failed], full["khat"][:K][~failed], equal_nan=True)
    live = ~full["excluded"]
    print("overall k-hat", overall, "threshold", thr, "cells above", int((plain["khat"][live] > thr).sum()), "matched", int((it > 0).sum()),
          "still above", int((full["khat"][live] > thr).sum()), "of the checked genes matched", int((xfull["iterations"] > 0).sum()))
    # a threshold that every cell exceeds: some cell takes a step
    low = fit.loo_moment_match_approximate_posterior(k_threshold=-1.0, max_iters=3)
    assert (low["iterations"] > 0).sum() >= 1 and np.all(low["iterations"] <= 3)
    assert np.all(low["khat"][low["iterations"] > 0] < low["khat_before"][low["iterations"] > 0])
    # the same bits on a second call, for a gene subset and for a permuted gene list
    again, xagain = fit.loo_moment_match_approximate_posterior(), fit.loo_predict_exact_moment_match_approximate_posterior()
    perm = np.random.default_rng(3).permutation(G)
    permuted = fit.loo_moment_match_approximate_posterior(perm)
    for k in KEYS:
        assert np.array_equal(again[k], full[k], equal_nan=True), k
        assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), k
        for sub in ([1], [2, 0], [40, 7, 0]):
            assert np.array_equal(fit.loo_moment_match_approximate_posterior(sub)[k], full[k][sub], equal_nan=True), (sub, k)
    xsub, xperm = fit.loo_predict_exact_moment_match_approximate_posterior([1]), fit.loo_predict_exact_moment_match_approximate_posterior([2, 0, 1])
    for k in XKEYS:
        assert np.array_equal(xagain[k], xfull[k], equal_nan=True), k
        assert np.array_equal(xsub[k], xfull[k][[1]], equal_nan=True), k
        assert np.array_equal(xperm[k], xfull[k][[2, 0, 1]], equal_nan=True), k
    none = fit.loo_moment_match_approximate_posterior(max_iters=0)
    for k in LOO4:
        assert np.array_equal(none[k], plain[k], equal_nan=True), k
    # refusals
    nuts = f["m"].fit_nuts(chains=2, iter=60, warmup=40, seed=1)
    given = f["m"].fit_from_draws(fit.draws())
    try:
        for other in (nuts, given):
            with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_moment_match_approx needs an ADVI fit"):
                other.loo_moment_match_approximate_posterior()
            with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_predict_exact_moment_match_approx needs an ADVI fit"):
                other.loo_predict_exact_moment_match_approximate_posterior()
    finally:
        nuts.close()
        given.close()
    for call in (fit.loo_moment_match_approximate_posterior, fit.loo_predict_exact_moment_match_approximate_posterior):
        with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
            call([0], k_threshold=np.nan)
        with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
            call([0], k_threshold=np.inf)
        with pytest.raises(_lib.PpcxError, match="max_iters must be >= 0"):
            call([0], max_iters=-1)
    with pytest.raises(_lib.PpcxError, match="gene out of range"):
        fit.loo_moment_match_approximate_posterior([G])
    with pytest.raises(_lib.PpcxError, match="gene out of range \\(a checked gene"):
        fit.loo_predict_exact_moment_match_approximate_posterior([K])
    with pytest.raises(_lib.PpcxError, match="need 0 < p_lo < p_hi < 1"):
        fit.loo_predict_exact_moment_match_approximate_posterior(p_lo=0.5, p_hi=0.5)
    # the NUTS entries keep refusing an ADVI fit, and name these
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_moment_match needs the draws of a NUTS fit.*ADVI fit.*ppcx_fit_loo_moment_match_approx"):
        fit.loo_moment_match()


def test_identify_outliers_with_each_modifier(bundled):
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=True,
              how_many_negative_controls=50, cores=1, seed=11, check_approximation_loo=True, exact_approximation_loo_intervals=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(df, **kw)
        first = identify_outliers(df, approximation_loo_moment_match=True, **kw)
        second = identify_outliers(df, exact_approximation_loo_moment_match=True, **kw)
    more = {"khat_before", "iterations", "scale", "shift", "k_threshold"}
    for out, changed in ((first, "approximation_loo"), (second, "exact_approximation_loo_intervals")):
        assert set(out.attrs) == set(plain.attrs)
        for col in plain.columns:
            assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
        for field in ("approximation_loo", "exact_approximation_loo_intervals"):
            for key in (field + "_discovery", field + "_test"):
                r, p = out.attrs[key], plain.attrs[key]
                if field != changed:
                    assert not more & set(r) and all(np.array_equal(r[k], p[k], equal_nan=True) for k in ("khat",)), key
                    continue
                assert more <= set(r) and not more & set(p) and r["scale"].shape == (3, 21, 3) and r["iterations"].shape == (3, 21), key
                assert np.array_equal(r["khat_before"], p["khat"], equal_nan=True), key
                it0 = r["iterations"] == 0
                for k in (LOO4 if field == "approximation_loo" else TEN):
                    assert np.array_equal(r[k][it0], p[k][it0], equal_nan=True), (key, k)
                print(key, "draws", r["n_draws"], "overall k-hat", r["khat_approximation"], "cells above the threshold",
                      int((p["khat"] > r["k_threshold"]).sum()), "matched", int((~it0).sum()), "still above", int((r["khat"] > r["k_threshold"]).sum()))
    with pytest.raises(ValueError, match="^approximation_loo_moment_match needs check_approximation_loo"):
        identify_outliers(df, **dict(kw, check_approximation_loo=False, approximation_loo_moment_match=True))
    with pytest.raises(ValueError, match="^exact_approximation_loo_moment_match needs exact_approximation_loo_intervals"):
        identify_outliers(df, **dict(kw, exact_approximation_loo_intervals=False, exact_approximation_loo_moment_match=True))
