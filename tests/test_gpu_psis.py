"""The Pareto-k diagnostic of ADVI fits on the MI355X (include/ppcx.h ppcx_fit_get_approximation / ppcx_fit_get_log_ratios /
ppcx_fit_psis): log_p at the kept draws against the oracle, log_g and k-hat against the numpy restatement
(tests/psis_restate.py), the kernel on known-k cases (testing build), refusals, determinism, and
identify_outliers(check_approximation=True)."""
import warnings

import numpy as np
import pytest

from tests import psis_restate as R
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library

pytestmark = pytest.mark.gpu


def compare_khat(got, ref, what):
    if np.isnan(ref):
        assert np.isnan(got), (what, got)
    elif np.isinf(ref):
        assert got == ref, (what, got, ref)
    else:
        assert abs(got - ref) <= 1e-12 * max(abs(ref), 1e-300), (what, got, ref)


def designs(bundled):
    """(name, counts, X, exposure, K, excl): the bundled testthat selection, a C = 3 factor design with excluded cells, a
    continuous covariate"""
    counts, X, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    yield "testthat 53x21", counts, X, libsize.mean() - libsize, K, None
    from ppcseq_amd.synth import synth
    d = synth(60, 12, K=4, seed=21, C=3)
    X3 = d["X"].copy()
    X3[:, 2] = (np.arange(12) % 3 == 0).astype(float)
    yield "factor C=3, exclusions", d["counts"], X3, d["exposure"], 4, np.array([5, 12 + 3, 3 * 12 + 11, 40 * 12], np.int32)
    d = synth(60, 12, K=4, seed=22)
    Xc = d["X"].copy()
    Xc[:, 1] = np.random.default_rng(22).normal(size=12)
    yield "continuous covariate", d["counts"], Xc, d["exposure"], 4, None


@pytest.fixture(scope="module")
def small():
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(40, 12, K=4, seed=3)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 4, device=0)
    yield m
    m.close()


def test_log_p_matches_oracle_and_log_g_matches_approximation(bundled, oracle):
    from ppcseq_amd import _lib
    for name, counts, X, expo, K, excl in designs(bundled):
        m = _lib.Model(counts, X, expo, K, excl=excl, device=0)
        try:
            f = m.fit_advi(output_samples=300, iter=2000, seed=4)
            try:
                lp, lg = f.log_ratios()
                mu, om = f.approximation()
                dr = f.draws()[0]
                assert lp.shape == lg.shape == (300,) and mu.shape == om.shape == (m.D,), name
                mo = oracle.model(counts, X, expo, K, excl=excl)
                for i in range(0, 300, 7):
                    lpo = oracle.log_prob_grad(mo, dr[i], want_grad=False)[0]
                    assert abs(lp[i] - lpo) <= 1e-11 * max(1.0, abs(lpo)), (name, i, lp[i], lpo)
                ref = R.log_g(dr, mu, om)
                assert np.all(np.abs(lg - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))), name
                # the approximation the draws came from: every coordinate, the six hyper-parameters included
                assert np.all(np.abs(dr.mean(axis=0) - mu) <= 5.0 * np.exp(om) / np.sqrt(300)), name
                assert np.all(np.abs(dr.std(axis=0) / np.exp(om) - 1.0) < 0.25), name
            finally:
                f.close()
        finally:
            m.close()


@pytest.mark.parametrize("n", [1000, 20000])
def test_psis_matches_restatement(small, n):
    """all D columns and column -1 against the restatement; 20 000 draws take the long-column path"""
    f = small.fit_advi(output_samples=n, iter=2000, seed=6)
    try:
        got = f.psis()
        assert np.array_equal(got["column"], np.r_[np.arange(small.D), -1])
        dr = f.draws()[0]
        r = R.log_ratios(*f.log_ratios())
        for d in range(small.D):
            compare_khat(got["khat"][d], R.khat(R.column_values(dr[:, d], r)), (n, d))
        compare_khat(got["khat"][-1], R.khat(r), (n, -1))
        assert np.isfinite(got["khat"][-1])
        again = f.psis()
        assert np.array_equal(got["khat"], again["khat"])                   # the same bits on every call
        pick = np.array([7, 0, small.D - 1, 3])
        sub = f.psis(pick, overall=False)
        assert np.array_equal(sub["column"], pick) and np.array_equal(sub["khat"], got["khat"][pick])
    finally:
        f.close()


def test_kernel_on_known_shapes():
    """the kernel itself (testing build) on GPD and normal-ratio samples, beside columns of the restatement's kind"""
    with testing_library() as _lib:
        rng = np.random.default_rng(0)
        for k in (0.3, 0.5, 0.9):
            r = np.log(R.gpd_sample(rng, k, 100_000))
            got = _lib.testing_psis(r)
            assert got.shape == (1,)
            compare_khat(got[0], R.khat(r), ("gpd", k))
            assert abs(got[0] - k) <= 0.1, (k, got[0])
        prev = -np.inf
        for s2 in (2.0, 4.0, 10.0):
            r = R.normal_ratios(np.random.default_rng(0), s2, 100_000)
            got = _lib.testing_psis(r)[0]
            compare_khat(got, R.khat(r), ("normal", s2))
            assert abs(got - (1 - 1 / s2)) <= 0.1 and got > prev, (s2, got)
            prev = got
        # columns: ordinary, with ties, with a NaN; ratios with -Inf entries; short and constant cases
        rng = np.random.default_rng(8)
        r = R.normal_ratios(rng, 3.0, 5000)
        r[::11] = -np.inf
        cols = rng.normal(size=(5000, 3))
        cols[:, 1] = np.round(cols[:, 1])
        cols[17, 2] = np.nan
        got = _lib.testing_psis(r, cols)
        for i in range(3):
            compare_khat(got[i], R.khat(R.column_values(cols[:, i], r)), ("column", i))
        assert np.isnan(got[2])
        compare_khat(got[3], R.khat(r), "ratios with -Inf")
        assert _lib.testing_psis(rng.normal(size=20))[0] == np.inf
        assert _lib.testing_psis(np.full(300, 2.0))[0] == np.inf
        for n in (224, 225, 4096, 4097):                                      # tail rules, the LDS path's limit
            r = R.normal_ratios(rng, 2.5, n)
            compare_khat(_lib.testing_psis(r)[0], R.khat(r), n)


def test_refusals(small):
    from ppcseq_amd import _lib
    f = small.fit_nuts(chains=2, iter=60, warmup=30, seed=5)
    try:
        for call in (lambda: f.psis([0]), f.log_ratios, f.approximation):
            with pytest.raises(_lib.PpcxError, match="ADVI"):
                call()
    finally:
        f.close()
    f = small.fit_from_draws(np.random.default_rng(0).normal(size=(1, 50, small.D)))
    try:
        with pytest.raises(_lib.PpcxError, match="ADVI"):
            f.psis()
    finally:
        f.close()
    a = small.fit_advi(output_samples=100, iter=500, seed=1)
    try:
        for bad in ([small.D], [-2]):
            with pytest.raises(_lib.PpcxError, match="out of range"):
                a.psis(bad, overall=False)
        assert a.psis([0])["khat"].shape == (2,)
    finally:
        a.close()


def test_psis_leaves_draws_and_ppc_unchanged(small):
    asked = small.fit_advi(output_samples=400, iter=1500, seed=9)
    try:
        k1 = asked.psis()
        d_asked = asked.draws()
        ppc_asked = asked.ppc(1.0, 0.05, 0.95, seed=3)
    finally:
        asked.close()
    plain = small.fit_advi(output_samples=400, iter=1500, seed=9)
    try:
        assert np.array_equal(plain.draws(), d_asked)
        assert np.array_equal(plain.ppc(1.0, 0.05, 0.95, seed=3), ppc_asked)
        assert np.array_equal(plain.psis()["khat"], k1["khat"])
    finally:
        plain.close()


def _bundled_frame(bundled):
    import pandas as pd
    genes = [str(g) for g in bundled["genes"]]
    samples = [str(s) for s in bundled["samples"]]
    G, S = len(genes), len(samples)
    df = pd.DataFrame({
        "symbol": np.repeat(genes, S), "sample": np.tile(samples, G), "value": bundled["value"].reshape(-1),
        "PValue": np.repeat(bundled["PValue"], S), "Label": np.tile(bundled["Label"].astype(str), G)})
    df["is_significant"] = df["symbol"].isin(["SLC16A12", "CYP1A1", "ART3"])
    return df


def test_identify_outliers_check_approximation(bundled):
    from ppcseq_amd.inference import approximation_warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=True,
              approximate_posterior_analysis=True, how_many_negative_controls=50, cores=1, seed=11)
    with warnings.catch_warnings(record=True) as w_plain:
        warnings.simplefilter("always")
        plain = identify_outliers(df, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = identify_outliers(df, check_approximation=True, **kw)
    assert "approximation_test" not in plain.attrs
    assert not any("Pareto k" in str(x.message) for x in w_plain)
    G = 53
    expect = []
    for key in ("approximation_discovery", "approximation_test"):
        a = out.attrs[key]
        assert np.array_equal(a["column"], np.r_[3 + G + np.arange(3), -1]), key
        assert a["khat"].shape == (4,) and not np.isnan(a["khat"]).any(), key
        expect += approximation_warnings(a["khat"][-1])
    got = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning) and "Pareto k" in str(x.message)]
    assert got == expect
    assert out["tot_deleterious_outliers"].tolist() == plain["tot_deleterious_outliers"].tolist() == [0, 1, 0]
