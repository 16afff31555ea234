"""The exact leave-one-out predictive under moment-matched weights on the device (Fit.loo_predict_exact_moment_match,
ppcx_fit_loo_predict_exact_moment_match): the designed draws of tests/loo_mm_cases.py reach the kernel through
Model.fit_from_draws and are held to the CPU build of its header (tests/loo_mm_exact_host); the draw counts at the ends of the
workgroup's stride and at the LDS / scratch hand-over, with the scratch in batches of two cells (testing build); the same fit's
other entries bit for bit; the truth case; and identify_outliers with the modifier on a short NUTS fit of the bundled case.

The entry takes checked genes only, and gene 1 of the tiny model of tests/loo_mm_cases.py is not one: checked_all() gives it a
slope column (small normal draws), so that both genes can be asked for; the CPU build reads the same gene. The one-gene truth
case (C = 1) gets an unused slope column in the same way.

Tolerances: integer fields equal, NaN and Inf in the same places; the rest against the CPU build at ten times the largest error
measured on the designed cells and the draw counts in units of max(1, |ref|), p_le / p_ge also relatively below 1e-3
(X.GPU_MEASURED; test_designed_cells_against_the_cpu_build and test_draw_counts print theirs), never above 1e-9."""
import numpy as np
import pytest

from tests import loo_mm_cases as cases
from tests import loo_mm_exact_restate as X
from tests.gpu_fixtures import testing_library
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

GPU_BOUND = min(10 * X.GPU_MEASURED, X.BOUND)
TC = 0.7352941
MM_KEYS = ("khat", "khat_before", "iterations", "scale", "shift")
TEN = ("mean", "sd", "p_le", "p_ge", "lower", "upper", "y", "excluded", "outside", "khat")
KEYS = TEN + ("pit_lt", "pit_le") + MM_KEYS[1:]


@pytest.fixture(scope="module")
def host():
    return X.host_lib()


def checked_all(ds):
    """the draw set with every gene a checked one: a slope column for each gene beyond K (C >= 2: normal draws of sd 0.3; C = 1:
    zeros, the column is not read)"""
    G = ds["counts"].shape[0]
    Cc = ds["X"].shape[1]
    assert Cc <= 2
    d = cases.dims(G, Cc, ds["K"])
    u = ds["draws"]
    rng = np.random.default_rng(17)
    extra = rng.normal(0.0, 0.3, (u.shape[0], G - ds["K"])) if Cc >= 2 else np.zeros((u.shape[0], G - ds["K"]))
    at = d["alpha1"] + ds["K"]
    out = dict(ds)
    out["draws"] = np.ascontiguousarray(np.concatenate([u[:, :at], extra, u[:, at:]], axis=1))
    out["K"] = G
    return out


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
    return np.concatenate([[res[k][i, s] for k in X.HEAD], res["scale"][i, s], res["shift"][i, s]]).astype(np.float64)


def _against_host(res, i, s, ref, what):
    """the device's cell against the CPU build's record: the integers and the places of NaN / Inf equal; returns the error of the rest"""
    got = _row(res, i, s)
    nan = np.isnan(ref[0])
    for k in X.INTEGERS:
        j = X.HEAD.index(k)
        if k in ("lower", "upper") and nan:
            assert got[j] == -1 and np.isnan(ref[j]), (what, k)         # the dict's integer for a NaN interval end
        elif k == "outside" and nan:
            assert got[j] == 0 and np.isnan(ref[j]), (what, k)
        else:
            assert got[j] == ref[j], (what, k, got[j], ref[j])
    real = [j for j in range(len(ref)) if j >= len(X.HEAD) or X.HEAD[j] in X.REALS]
    assert np.array_equal(np.isnan(got[real]), np.isnan(ref[real])) and np.array_equal(np.isinf(got[real]), np.isinf(ref[real])), (what, got, ref)
    Cc = (len(ref) - len(X.HEAD)) // 2 - 1
    as_ref = dict(zip(X.HEAD, ref[:len(X.HEAD)]), scale=ref[len(X.HEAD):len(X.HEAD) + Cc + 1], shift=ref[len(X.HEAD) + Cc + 1:])
    return X.errors(got, as_ref)


def test_designed_cells_against_the_cpu_build(host):
    held, sets = {}, {}
    worst, matched = 0.0, 0
    try:
        for c in cases.designed():
            if c["set"] not in held:
                sets[c["set"]] = checked_all(cases.draw_set(c["set"]))
                held[c["set"]] = _Held(sets[c["set"]])
            ds, fit = sets[c["set"]], held[c["set"]].fit
            S = ds["counts"].shape[1]
            kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"], truncation_compensation=TC)
            res = fit.loo_predict_exact_moment_match([c["g"]], r_eff=np.full((1, S), c["r_eff"]), **kw)
            assert res["k_threshold"] == c["k_threshold"] and res["iterations"].dtype == np.int64 and res["scale"].shape == (1, S, 3)
            gene = cases.gene_of(ds, c["g"])
            for s in range(S):                                            # the designed cell and its gene's other cells
                ref = X.host_cell(host, gene, s, r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"], tc=TC)
                err = _against_host(res, 0, s, ref, (c["name"], s))
                worst = max(worst, err)
                assert err <= GPU_BOUND, (c["name"], s, err)
                matched += ref[11] > 0
    finally:
        for h in held.values():
            h.close()
    print("cells matched", int(matched), "largest error against the CPU build:", worst)
    assert matched >= 8
    assert worst <= X.GPU_MEASURED                                    # the recorded value is the measured one


@pytest.mark.parametrize("n", [1, 4, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097])
def test_draw_counts(host, n):
    """the ends of the workgroup's stride and the LDS / scratch hand-over; the scratch bound set so that the scratch path runs
    in batches of two cells (and the gene table in batches of two genes)"""
    ds = cases.prefix(checked_all(cases.long_set()), n)
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_predict_exact_moment_match(k_threshold=0.7)     # (loo_threshold is not defined at one draw)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)
            try:
                res = h.fit.loo_predict_exact_moment_match(k_threshold=0.7)
                mm = h.fit.loo_moment_match(np.arange(2), k_threshold=0.7)
                plain = h.fit.loo_predict_exact()
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in KEYS:
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    for k in MM_KEYS:
        assert np.array_equal(res[k], mm[k], equal_nan=True), k        # the matching's own record
    it0 = res["iterations"] == 0
    for k in TEN:
        assert np.array_equal(res[k][it0], plain[k][it0], equal_nan=True), k
    matched, worst = 0, 0.0
    for g in range(2):
        gene = cases.gene_of(ds, g)
        for s in range(4):
            ref = X.host_cell(host, gene, s, k_threshold=0.7)
            err = _against_host(res, g, s, ref, (n, g, s))
            worst = max(worst, err)
            assert err <= GPU_BOUND, (n, g, s, err)
            matched += res["iterations"][g, s] > 0
    print("n", n, "cells matched", int(matched), "largest error against the CPU build", worst)
    assert matched >= (1 if n >= 63 else 0)
    assert worst <= X.GPU_MEASURED


def test_against_the_fits_other_entries():
    """on the draws of set "c" with both genes checked (one excluded cell, cells that are matched and cells that are not)"""
    from ppcseq_amd import _lib
    from ppcseq_amd.inference import loo_threshold
    h = _Held(checked_all(cases.draw_set("c")))
    try:
        fit = h.fit
        G, S = 2, 4
        kw = dict(truncation_compensation=TC, p_lo=0.01, p_hi=0.9)
        full = fit.loo_predict_exact_moment_match(**kw)
        mm, plain, ppc = fit.loo_moment_match(np.arange(G)), fit.loo_predict_exact(**kw), fit.ppc_exact(**kw)
        assert full["k_threshold"] == loo_threshold(1000) and full["n_draws"] == 1000 and list(full["genes"]) == [0, 1]
        assert full["scale"].shape == (G, S, 3) and full["mean"].shape == (G, S) and full["iterations"].dtype == np.int64
        it = full["iterations"]
        assert (it > 0).sum() >= 2 and (it == 0).sum() >= 2 and full["excluded"].sum() == 1
        for k in MM_KEYS:
            assert np.array_equal(full[k], mm[k], equal_nan=True), k
        assert np.all(full["khat"][it > 0] < full["khat_before"][it > 0]) and np.all(np.isfinite(full["mean"]))
        for k in TEN + ("pit_lt", "pit_le"):
            assert np.array_equal(full[k][it == 0], plain[k][it == 0], equal_nan=True), k
        for k in ("mean", "sd", "khat"):
            assert np.all(full[k][it > 0] != plain[k][it > 0]), k          # a matched cell is not plain PSIS's
        ex = full["excluded"]
        for k in TEN[:9]:
            assert np.array_equal(full[k][ex], ppc[k][ex], equal_nan=True), k
        assert np.all(np.isnan(full["khat"][ex])) and np.all(it[ex] == 0)
        # the same bits on a second call, for a gene subset and for a permuted gene list
        again, sub, perm = fit.loo_predict_exact_moment_match(**kw), fit.loo_predict_exact_moment_match([1], **kw), \
            fit.loo_predict_exact_moment_match([1, 0], **kw)
        for k in KEYS:
            assert np.array_equal(again[k], full[k], equal_nan=True), k
            assert np.array_equal(sub[k], full[k][[1]], equal_nan=True), k
            assert np.array_equal(perm[k], full[k][[1, 0]], equal_nan=True), k
        auto = fit.loo_predict_exact_moment_match(r_eff="auto", **kw)
        mm_auto = fit.loo_moment_match(np.arange(G), r_eff="auto")
        assert auto["r_eff"].shape == (G, S) and np.array_equal(auto["r_eff"], mm_auto["r_eff"])
        for k in MM_KEYS:
            assert np.array_equal(auto[k], mm_auto[k], equal_nan=True), k
        none = fit.loo_predict_exact_moment_match(max_iters=0, **kw)
        for k in TEN + ("pit_lt", "pit_le"):
            assert np.array_equal(none[k], plain[k], equal_nan=True), k
        assert np.all(none["iterations"] == 0) and np.all(none["scale"] == 1.0) and np.all(none["shift"] == 0.0)
        # refusals
        with pytest.raises(_lib.PpcxError, match="need 0 < p_lo < p_hi < 1"):
            fit.loo_predict_exact_moment_match(p_lo=0.5, p_hi=0.5)
        with pytest.raises(_lib.PpcxError, match="need 0 < p_lo < p_hi < 1"):
            fit.loo_predict_exact_moment_match(p_lo=0.0, p_hi=0.9)
        with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
            fit.loo_predict_exact_moment_match([0], k_threshold=np.inf)
        with pytest.raises(_lib.PpcxError, match="max_iters must be >= 0"):
            fit.loo_predict_exact_moment_match([0], max_iters=-1)
        with pytest.raises(_lib.PpcxError, match="truncation_compensation must be finite and > 0"):
            fit.loo_predict_exact_moment_match([0], truncation_compensation=0.0)
        with pytest.raises(_lib.PpcxError, match="r_eff"):
            fit.loo_predict_exact_moment_match([0], r_eff=np.zeros((1, S)))
        advi = h.m.fit_advi(output_samples=200, iter=1000, seed=4)
        try:
            with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_predict_exact_moment_match needs the draws of a NUTS fit.*ADVI fit"):
                advi.loo_predict_exact_moment_match()
        finally:
            advi.close()
    finally:
        h.close()
    h = _Held(cases.draw_set("c"))                                     # K = 1: gene 1 is not a checked gene
    try:
        with pytest.raises(_lib.PpcxError, match="gene out of range \\(a checked gene"):
            h.fit.loo_predict_exact_moment_match([1])
        assert h.fit.loo_predict_exact_moment_match()["mean"].shape == (1, 4)
    finally:
        h.close()


def test_truth_case(host):
    """n = 1000, seed 1: the device gives the CPU build's figures (tests/test_loo_mm_exact_host.py holds those to the truth)"""
    ds = checked_all(cases.truth_set(1, 1000))
    h = _Held(ds)
    try:
        res = h.fit.loo_predict_exact_moment_match()
    finally:
        h.close()
    s = cases.TRUTH_CELL
    ref = X.host_cell(host, cases.gene_of(ds, 0), s)
    err = _against_host(res, 0, s, ref, "truth")
    print("truth case: khat", res["khat_before"][0, s], "->", res["khat"][0, s], "mean", res["mean"][0, s], "upper", res["upper"][0, s],
          "p_ge", res["p_ge"][0, s], "error against the CPU build", err)
    assert err <= GPU_BOUND and ref[11] == 2 and res["khat"][0, s] < 0.7 <= res["khat_before"][0, s]
    assert abs(res["mean"][0, s] - 146.9) < 0.1 and res["upper"][0, s] == 327


def test_identify_outliers_with_the_modifier(bundled):
    """a short NUTS run of the bundled 53 x 21 case: the attrs are present, flags and frame are those of the call without the two
    options; how many cells were matched and how many `outside` verdicts changed is printed, not asserted"""
    import warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11,
              adj_prob_theshold_2=0.01)                     # 1 000 draws in the second pass too: the test stays short
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        bare = identify_outliers(df, **kw)
        plain = identify_outliers(df, exact_loo_intervals=True, **kw)
        out = identify_outliers(df, exact_loo_intervals=True, exact_loo_moment_match=True, **kw)
    assert set(out.attrs) == set(plain.attrs) == set(bare.attrs) | {"exact_loo_intervals_discovery", "exact_loo_intervals_test"}
    for col in bare.columns:
        assert repr(bare[col].tolist()) == repr(out[col].tolist()), col
    for key in ("exact_loo_intervals_discovery", "exact_loo_intervals_test"):
        r, p = out.attrs[key], plain.attrs[key]
        assert {"khat_before", "iterations", "scale", "shift", "k_threshold"} <= set(r) and "khat_before" not in p
        assert r["scale"].shape == (3, 21, 3) and r["iterations"].shape == (3, 21)
        assert np.array_equal(r["khat_before"], p["khat"], equal_nan=True)
        it = r["iterations"]
        for k in TEN:
            assert np.array_equal(r[k][it == 0], p[k][it == 0], equal_nan=True), (key, k)
        print(key, "draws", r["n_draws"], "cells above the threshold", int((p["khat"] > r["k_threshold"]).sum()), "matched", int((it > 0).sum()),
              "still above", int((r["khat"] > r["k_threshold"]).sum()), "outside verdicts changed", int((r["outside"] != p["outside"]).sum()),
              "outside before", int(p["outside"].sum()), "after", int(r["outside"].sum()))
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals"):
        identify_outliers(df, exact_loo_moment_match=True, **kw)
