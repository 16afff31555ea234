"""Gene-local moment matching of PSIS-LOO cells on the device (Fit.loo_moment_match, ppcx_fit_loo_moment_match): the designed
draws of tests/loo_mm_cases.py reach the kernel through Model.fit_from_draws and are held to the CPU build of its header
(tests/loo_mm_host); the draw counts at the ends of the workgroup's stride and at the LDS / scratch hand-over, with the scratch in
batches of two cells (testing build); the truth case; a short NUTS fit of the bundled 53 x 21 case with two excluded cells; and
identify_outliers with the modifier.

Tolerances: iterations equal, NaN and Inf in the same places, the cells with iterations = 0 bit-equal to Fit.loo; khat, elpd_loo,
scale and shift against the CPU build at ten times the largest error measured on the designed cells and the draw counts in units
of max(1, |ref|) (R.GPU_MEASURED; test_designed_cells_against_the_cpu_build and test_draw_counts print theirs), never above 1e-9."""
import numpy as np
import pytest

from tests import loo_mm_cases as cases
from tests import loo_mm_restate as R
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

GPU_BOUND = min(10 * R.GPU_MEASURED, R.BOUND)


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


class _Held:
    """a draw set as a model and a fit over its draws"""

    def __init__(self, ds):
        from ppcseq_amd import _lib
        self.m = _lib.Model(ds["counts"], ds["X"], ds["expo"], ds["K"], lambda_mu_mu=ds["lambda_mu_mu"],
                            excl=np.asarray(ds["excl"], np.int32), device=0)
        self.fit = self.m.fit_from_draws(np.ascontiguousarray(ds["draws"][None]))

    def close(self):
        self.fit.close()
        self.m.close()


def _row(res, i, s):
    return np.concatenate([[res[k][i, s] for k in R.HEAD], res["scale"][i, s], res["shift"][i, s]]).astype(np.float64)


def _against_host(got, ref, what):
    assert got[5] == ref[5], (what, got[5], ref[5])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, got, ref)
    return R.errors(got, ref)


def test_designed_cells_against_the_cpu_build(host):
    held = {}
    worst = 0.0
    try:
        for c in cases.designed():
            ds = cases.draw_set(c["set"])
            if c["set"] not in held:
                held[c["set"]] = _Held(ds)
            fit = held[c["set"]].fit
            S = ds["counts"].shape[1]
            kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
            re = np.full((1, S), c["r_eff"])
            res = fit.loo_moment_match([c["g"]], r_eff=re, **kw)
            plain = fit.loo([c["g"]], r_eff=re)
            ref, _ = R.host_cell(host, cases.gene_of(ds, c["g"]), c["s"], r_eff=c["r_eff"], **kw)
            got = _row(res, 0, c["s"])
            err = _against_host(got, ref, c["name"])
            worst = max(worst, err)
            assert err <= GPU_BOUND, (c["name"], err)
            assert res["k_threshold"] == c["k_threshold"] and res["iterations"].dtype == np.int64
            for s in range(S):                                            # untouched cells: Fit.loo's bits
                if res["iterations"][0, s] == 0:
                    assert all(np.array_equal(res[k][0, s], plain[k][0, s], equal_nan=True) for k in ("elpd_loo", "p_loo", "looic", "khat")), (c["name"], s)
                    assert np.array_equal(res["khat_before"][0, s], plain["khat"][0, s], equal_nan=True)
                    assert np.all(res["scale"][0, s] == 1.0) and np.all(res["shift"][0, s] == 0.0)
                else:
                    assert res["khat"][0, s] < res["khat_before"][0, s] and res["khat_before"][0, s] == plain["khat"][0, s]
    finally:
        for h in held.values():
            h.close()
    print("largest error of khat, elpd_loo, scale, shift against the CPU build:", worst)
    assert worst <= R.GPU_MEASURED                                    # the recorded value is the measured one


@pytest.mark.parametrize("n", [1, 4, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097])
def test_draw_counts(host, n):
    """the ends of the workgroup's stride and the LDS / scratch hand-over; the scratch bound set so that the scratch path runs
    in batches of two cells (and the gene table in batches of two genes)"""
    ds = cases.prefix(cases.long_set(), n)
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_moment_match(k_threshold=0.7)        # (loo_threshold is not defined at one draw)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)
            try:
                res = h.fit.loo_moment_match(k_threshold=0.7)
                plain = h.fit.loo()
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in R.HEAD + ("scale", "shift"):
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    matched, worst = 0, 0.0
    for g in range(2):
        gene = cases.gene_of(ds, g)
        for s in range(4):
            ref, _ = R.host_cell(host, gene, s, k_threshold=0.7)
            err = _against_host(_row(res, g, s), ref, (n, g, s))
            worst = max(worst, err)
            assert err <= GPU_BOUND, (n, g, s, err)
            if res["iterations"][g, s] == 0:
                assert all(np.array_equal(res[k][g, s], plain[k][g, s], equal_nan=True) for k in ("elpd_loo", "p_loo", "looic", "khat"))
            matched += res["iterations"][g, s] > 0
    print("n", n, "cells matched", int(matched), "largest error against the CPU build", worst)
    assert matched >= (1 if n >= 63 else 0)


@pytest.mark.parametrize("n", [1000, 4000])
def test_truth_case(n):
    truth = cases.truth_elpd()
    for seed in (1, 2, 3):
        h = _Held(cases.truth_set(seed, n))
        try:
            res, plain = h.fit.loo_moment_match(), h.fit.loo()
        finally:
            h.close()
        s = cases.TRUTH_CELL
        e0, e1 = abs(plain["elpd_loo"][0, s] - truth), abs(res["elpd_loo"][0, s] - truth)
        print(n, seed, "error of elpd_loo: plain PSIS", e0, "matched", e1, "khat", res["khat_before"][0, s], "->", res["khat"][0, s])
        assert res["khat"][0, s] < 0.7 <= res["khat_before"][0, s], (n, seed)
        assert e1 <= 0.5 * e0, (n, seed)


EXCL = (0 * 21 + 3, 2 * 21 + 20)                     # the two cells the model holds out
KEYS = R.HEAD + ("scale", "shift")


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X, expo, K, excl=np.array(EXCL, np.int32), device=0)
    nuts = m.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    yield dict(m=m, counts=counts, X=X, expo=expo, K=K, nuts=nuts, advi=advi)
    nuts.close()
    advi.close()
    m.close()


def test_nuts_fit(fits):
    from ppcseq_amd import _lib
    f = fits
    fit = f["nuts"]
    full, plain = fit.loo_moment_match(), fit.loo()
    thr = full["k_threshold"]
    from ppcseq_amd.inference import loo_threshold
    assert thr == loo_threshold(fit.chains * fit.n_keep) and full["n_draws"] == 450
    G, S = f["counts"].shape
    assert full["scale"].shape == (G, S, 3) and full["elpd_loo"].shape == (G, S) and full["excluded"].sum() == 2
    live = ~full["excluded"]
    assert np.all(full["khat"][live] <= full["khat_before"][live])
    it = full["iterations"]
    assert np.all(full["khat_before"][it > 0] > thr) and np.all(it >= 0) and np.all(it <= 30)
    assert np.array_equal(full["khat_before"], plain["khat"], equal_nan=True)
    for k in ("elpd_loo", "p_loo", "looic", "khat"):
        assert np.array_equal(full[k][it == 0], plain[k][it == 0], equal_nan=True), k
    assert np.all(full["scale"][it == 0] == 1.0) and np.all(full["shift"][it == 0] == 0.0)
    assert np.all(full["scale"][f["K"]:, :, 1] == 1.0) and np.all(full["shift"][f["K"]:, :, 1] == 0.0)    # genes without a slope
    assert np.all(np.isfinite(full["elpd_loo"]))
    print("cells above the threshold", int((plain["khat"][live] > thr).sum()), "matched", int((it > 0).sum()), "still above",
          int((full["khat"][live] > thr).sum()))
    # the same bits on a second call, for a gene subset and for a permuted gene list
    again = fit.loo_moment_match()
    perm = np.random.default_rng(3).permutation(G)
    permuted = fit.loo_moment_match(perm)
    for sub in ([1], [2, 0], [40, 7, 0]):
        r = fit.loo_moment_match(sub)
        for k in KEYS:
            assert np.array_equal(r[k], full[k][sub], equal_nan=True), (sub, k)
    for k in KEYS:
        assert np.array_equal(again[k], full[k], equal_nan=True), k
        assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), k
    auto = fit.loo_moment_match(np.arange(f["K"]), r_eff="auto")
    assert auto["r_eff"].shape == (f["K"], S) and np.all(auto["khat"][~auto["excluded"]] <= auto["khat_before"][~auto["excluded"]])
    none = fit.loo_moment_match(max_iters=0)
    for k in ("elpd_loo", "p_loo", "looic", "khat"):
        assert np.array_equal(none[k], plain[k], equal_nan=True), k
    # refusals
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_moment_match needs the draws of a NUTS fit.*ADVI fit"):
        f["advi"].loo_moment_match()
    with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
        fit.loo_moment_match([0], k_threshold=np.nan)
    with pytest.raises(_lib.PpcxError, match="max_iters must be >= 0"):
        fit.loo_moment_match([0], max_iters=-1)
    with pytest.raises(_lib.PpcxError, match="gene out of range"):
        fit.loo_moment_match([G])
    with pytest.raises(_lib.PpcxError, match="r_eff"):
        fit.loo_moment_match([0], r_eff=np.zeros((1, S)))
    # recorded, not asserted: the matched cell with the highest khat_before, refitted with that cell held out
    cand = np.where(it > 0, full["khat_before"], -np.inf)
    if np.isfinite(cand.max()):
        g, s = np.unravel_index(np.argmax(cand), cand.shape)
        m2 = _lib.Model(f["counts"], f["X"], f["expo"], f["K"], excl=np.array(EXCL + (g * S + s,), np.int32), device=0)
        try:
            refit = m2.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
            try:
                held_out = refit.loo([g])["elpd_loo"][0, s]
            finally:
                refit.close()
        finally:
            m2.close()
        print("cell", (int(g), int(s)), "elpd_loo plain", plain["elpd_loo"][g, s], "matched", full["elpd_loo"][g, s], "refit", held_out,
              "khat", full["khat_before"][g, s], "->", full["khat"][g, s], "iterations", int(it[g, s]))


def test_identify_outliers_with_the_modifier(bundled):
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11,
              adj_prob_theshold_2=0.01)                     # 1 000 draws in the second pass too: the test stays short
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = identify_outliers(df, check_loo=True, **kw)
        out = identify_outliers(df, check_loo=True, loo_moment_match=True, **kw)
    assert set(out.attrs) == set(plain.attrs)
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    for key in ("loo_discovery", "loo_test"):
        r, p = out.attrs[key], plain.attrs[key]
        assert {"khat_before", "iterations", "scale", "shift", "k_threshold"} <= set(r) and "khat_before" not in p
        assert r["scale"].shape == (3, 21, 3) and r["iterations"].shape == (3, 21)
        assert np.array_equal(r["khat_before"], p["khat"], equal_nan=True)
        assert np.all(r["khat"][~r["excluded"]] <= p["khat"][~p["excluded"]])
    with pytest.raises(ValueError, match="^loo_moment_match needs check_loo"):
        identify_outliers(df, loo_moment_match=True, **kw)
