"""The leave-one-out predictive interval and LOO-PIT per observed cell on the MI355X (include/ppcx.h ppcx_fit_loo_predict): the
kernel on designed columns (testing build), a fit loaded from the oracle's NUTS draws against the numpy restatement
(tests/loo_predict_restate.py), excluded cells against Fit.ppc bit for bit, k-hat against Fit.loo bit for bit, determinism,
refusals and identify_outliers(check_loo_intervals).

Tolerances (tests/loo_predict_restate.check): sums of weights 1e-12 max(1, |ref|); a quantile lies between the restatement's
support points and within 1e-12 max(1, |ref|) + 1e-12 (v* - v-) / (F(v*) - F(v-)); khat 1e-12 max(1, |ref|). Cells that
`borderline` marks are skipped for lower / upper only, at most 1 cell in 1 000 per test."""
import warnings

import numpy as np
import pytest

from tests import loo_predict_cases as cases
from tests import loo_predict_restate as R
from tests.gpu_fixtures import testing_library
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu


def _slice_doubles(n):
    return 2 * n + (n + 1) // 2                          # ratios, weights, counts of one cell on the scratch path


def test_kernel_on_designed_columns():
    with testing_library() as _lib:
        for c in cases.designed():
            kw = dict(r_eff=c["r_eff"], excluded=c["excluded"], p_lo=c["p_lo"], p_hi=c["p_hi"])
            ref = R.point(c["ll"], c["x"], c["y"], **kw)
            got = _lib.testing_loo_predict(c["ll"][:, None], c["x"][:, None], [c["y"]], [int(c["excluded"])], [c["r_eff"]],
                                           c["p_lo"], c["p_hi"])[0]
            print(c["name"], got, [ref[k] for k in R.FIELDS])
            exact = c.get("exact_upper", False)
            skipped = R.check(got, ref, None if exact else c["ll"], c["x"], c["r_eff"], c["p_lo"], c["p_hi"], c["name"])
            assert skipped == 0, c["name"]
            if c["excluded"] and np.isfinite(got[0]):                    # integer sums and one fma: exact
                assert got[0] == ref["mean"] and got[1] == ref["lower"] and got[2] == ref["upper"], c["name"]
                assert got[3] == ref["pit_lt"] and got[4] == ref["pit_le"], c["name"]
        # several columns in one launch are the columns one by one
        cs = [c for c in cases.designed() if c["ll"].size == 1000 and c["p_lo"] == 0.025 and c["p_hi"] == 0.975]
        assert len(cs) >= 6
        ll = np.stack([c["ll"] for c in cs], axis=1)
        x = np.stack([c["x"] for c in cs], axis=1)
        args = ([c["y"] for c in cs], [int(c["excluded"]) for c in cs], [c["r_eff"] for c in cs])
        both = _lib.testing_loo_predict(ll, x, *args)
        for i, c in enumerate(cs):
            one = _lib.testing_loo_predict(ll[:, i:i + 1], x[:, i:i + 1], *[a[i:i + 1] for a in args])
            assert np.array_equal(both[i], one[0], equal_nan=True), c["name"]
        # columns at the end of the LDS path and beyond, and the scratch in several batches, give the same bits as one batch
        for n in (4096, 4097, 9000):
            ll, x, y = cases.long_columns(n)
            one = _lib.testing_loo_predict(ll, x, y)
            for i in range(ll.shape[1]):
                assert R.check(one[i], R.point(ll[:, i], x[:, i], y[i]), ll[:, i], x[:, i], what=(n, i)) == 0
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * _slice_doubles(n) + 8)         # two cells per batch
            try:
                assert np.array_equal(_lib.testing_loo_predict(ll, x, y), one, equal_nan=True), n
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        with pytest.raises(_lib.PpcxError, match="p_lo"):
            _lib.testing_loo_predict(np.zeros((30, 1)), np.ones((30, 1)), [1], p_lo=0.5, p_hi=0.5)


@pytest.fixture(scope="module")
def oracle_fit(oracle):
    from ppcseq_amd import _lib
    f = cases.fit_inputs(oracle)
    d = f["d"]
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=f["excl"], device=0)
    fit = m.fit_from_draws(f["draws"])
    yield m, fit, f
    fit.close()
    m.close()


def test_fit_matches_restatement(oracle_fit):
    m, fit, f = oracle_fit
    d, x = f["d"], f["x"]
    G, S = m.G, m.S
    ll = fit.log_lik().reshape(-1, G, S)
    assert np.abs(ll - f["ll"]).max() <= 1e-9                            # the device's log-likelihood is the scipy one
    ci, rng = fit.ppc(1.0, 0.025, 0.975, seed=cases.FIT_SEED, return_counts_rng=True)
    assert np.array_equal(rng, x[:, :4])                                 # g < K: the integers of counts_rng
    rng_r = np.random.default_rng(0)
    for r_eff in (None, rng_r.uniform(0.2, 1.5, size=(G, S))):
        res = fit.loo_predict(seed=cases.FIT_SEED, r_eff=r_eff)
        skipped = 0
        for g in range(G):
            for s in range(S):
                excl = g * S + s in cases.FIT_EXCL
                assert bool(res["excluded"][g, s]) == excl
                re = 1.0 if r_eff is None else r_eff[g, s]
                ref = R.point(ll[:, g, s], x[:, g, s], int(d["counts"][g, s]), r_eff=re, excluded=excl)
                got = [res[k][g, s] for k in R.FIELDS]
                skipped += R.check(got, ref, ll[:, g, s], x[:, g, s], re, what=(g, s)) > 0
        print("cells skipped as borderline:", skipped)
        assert skipped <= G * S / 1000
        assert np.array_equal(res["y"], d["counts"])
        assert np.array_equal(res["outside"], (res["y"] < res["lower"]) | (res["y"] > res["upper"]))


def test_excluded_cells_equal_ppc_bit_for_bit(oracle_fit):
    m, fit, f = oracle_fit
    for tc, p, seed in ((1.0, 0.025, 5), (0.7352941, 0.002, 11)):
        ci = fit.ppc(tc, p, 1 - p, seed=seed)
        res = fit.loo_predict(np.arange(m.K), p_lo=p, p_hi=1 - p, seed=seed, truncation_compensation=tc)
        assert res["excluded"].sum() == 2
        for g, s in ((0, 3), (1, 7)):
            assert res["excluded"][g, s]
            assert res["mean"][g, s] == ci[g, s, 0] and res["lower"][g, s] == ci[g, s, 2] and res["upper"][g, s] == ci[g, s, 3]
            assert np.isnan(res["khat"][g, s])


def test_khat_is_loo_s_and_fields_are_ordered(oracle_fit):
    m, fit, f = oracle_fit
    re = np.random.default_rng(1).uniform(0.3, 1.4, size=(m.G, m.S))
    for r_eff in (None, re):
        a, b = fit.loo_predict(r_eff=r_eff), fit.loo(r_eff=r_eff)
        assert np.array_equal(a["khat"], b["khat"], equal_nan=True)
        assert np.all(a["pit_lt"] <= a["pit_le"]) and np.all(a["lower"] <= a["upper"])
        assert np.all(a["pit_lt"] >= 0) and np.all(a["pit_le"] <= 1 + 1e-12)
    # the truncation compensation scales the predictive draws only: the weights' k-hat does not move
    c = fit.loo_predict(truncation_compensation=0.7352941)
    assert np.array_equal(c["khat"], fit.loo()["khat"], equal_nan=True)
    assert not np.array_equal(c["upper"], fit.loo_predict()["upper"])


def test_determinism_subsets_and_batches(oracle_fit):
    m, fit, f = oracle_fit
    a, b = fit.loo_predict(seed=3), fit.loo_predict(seed=3)
    sub = np.array([7, 0, 29, 4])
    s = fit.loo_predict(sub, seed=3)
    g = m.fit_from_draws(fit.draws())
    try:
        c = g.loo_predict(seed=3)
    finally:
        g.close()
    for k in R.FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(s[k], a[k][sub], equal_nan=True), k
        assert np.array_equal(c[k], a[k], equal_nan=True), k
    assert not np.array_equal(fit.loo_predict(seed=4)["mean"], a["mean"])
    d = f["d"]
    with testing_library() as _lib:
        mt = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=f["excl"], device=0)
        try:
            ft = mt.fit_from_draws(f["draws"])
            try:
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * 1000 + 8)      # the gene table in batches of one or two genes
                try:
                    got = ft.loo_predict(seed=3)
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
            finally:
                ft.close()
        finally:
            mt.close()
    for k in R.FIELDS:
        assert np.array_equal(got[k], a[k], equal_nan=True), k


def test_refusals(oracle_fit):
    from ppcseq_amd import _lib
    m, fit, f = oracle_fit
    for bad in ([m.G], [-1]):
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            fit.loo_predict(bad)
    for r in (0.0, -1.0, np.nan, np.inf):
        re = np.ones((2, m.S)); re[1, 3] = r
        with pytest.raises(_lib.PpcxError, match="r_eff"):
            fit.loo_predict([0, 1], r_eff=re)
    for lo, hi in ((-0.1, 0.9), (0.5, 0.5), (0.6, 0.4), (0.1, 1.1), (np.nan, 0.9)):
        with pytest.raises(_lib.PpcxError, match="p_lo"):
            fit.loo_predict([0], p_lo=lo, p_hi=hi)
    for tc in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_lib.PpcxError, match="truncation_compensation"):
            fit.loo_predict([0], truncation_compensation=tc)
    a = m.fit_advi(output_samples=100, iter=500, seed=1)
    try:
        with pytest.raises(_lib.PpcxError, match="NUTS"):
            a.loo_predict()
    finally:
        a.close()


def test_identify_outliers_check_loo_intervals(bundled):
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11)
    plain = identify_outliers(df, **kw)
    off = identify_outliers(df, check_loo_intervals=False, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = identify_outliers(df, check_loo_intervals=True, just_discovery=False, **kw)
    disc = identify_outliers(df, check_loo_intervals=True, just_discovery=True, **kw)
    assert not [x for x in w if "Pareto k" in str(x.message)]             # the k-hat warnings are check_loo's
    assert "loo_intervals_test" not in plain.attrs and "loo_intervals_test" not in off.attrs
    assert sorted(plain.attrs) == sorted(off.attrs)
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(off[col].tolist()), col
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    K, S = 3, 21
    for key in ("loo_intervals_discovery", "loo_intervals_test"):
        r = out.attrs[key]
        for k in R.FIELDS + ("excluded", "y", "outside"):
            assert r[k].shape == (K, S), (key, k)
        assert np.all(np.isfinite(r["mean"])) and np.all(r["lower"] <= r["upper"]), key
    assert out.attrs["loo_intervals_discovery"]["excluded"].sum() == 0
    assert out.attrs["loo_intervals_test"]["excluded"].sum() >= 1          # the discovery pass's outliers are held out
    assert out["tot_deleterious_outliers"].tolist() == plain["tot_deleterious_outliers"].tolist()
    # the discovery pass's flagged cells against their leave-one-out intervals (reported, see the pull request)
    li = disc.attrs["loo_intervals_discovery"]
    col = disc["deleterious_outliers"] if "deleterious_outliers" in disc.columns else ~disc["ppc"]   # what pass 2 excludes
    flagged = col.to_numpy().astype(bool).reshape(K, S)
    for g, s in zip(*np.nonzero(flagged)):
        print("flagged cell", g, s, "y", li["y"][g, s], "khat", li["khat"][g, s], "loo interval", li["lower"][g, s],
              li["upper"][g, s], "outside", li["outside"][g, s])
    trusted = flagged & (li["khat"] <= 0.7)
    assert np.all(li["outside"][trusted])
