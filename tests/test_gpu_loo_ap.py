"""PSIS-LOO per observed cell of an ADVI fit on the MI355X (include/ppcx.h ppcx_fit_loo_approx / ppcx_fit_loo_predict_approx;
loo::loo_approximate_posterior): a small fit against the numpy restatement (tests/loo_ap_restate.py) on inputs of identical bits,
the kernels on designed columns (testing build), the LDS path against the scratch path and its batches, the predictive interval
and LOO-PIT under the same weights, refusals and identify_outliers(check_approximation_loo, check_approximation_loo_intervals).

Tolerances: 1e-12 max(1, |ref|) for the LOO fields (tests/test_gpu_loo._compare); those of tests/loo_predict_restate.check for the
predictive fields, with at most 1 cell in 1 000 skipped as borderline (tests/test_gpu_loo_predict.py)."""
import warnings

import numpy as np
import pytest

from tests import loo_ap_cases as cases
from tests import loo_ap_restate as A
from tests import loo_predict_restate as R
from tests import loo_restate as L
from tests import psis_restate as P
from tests.test_gpu_loo import _compare
from tests.gpu_fixtures import testing_library
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

EXCL = (3, 17)
SEED = 5                                                        # of the predictive draws


@pytest.fixture(scope="module")
def small_advi():
    """(model, ADVI fit, synth data, ll [n, G S] at the fit's draws, a [n]): the reference's inputs are the device's own bits"""
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(30, 10, K=4, seed=5)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=np.array(EXCL, np.int32), device=0)
    f = m.fit_advi(output_samples=1000, iter=2000, seed=3)
    g = m.fit_from_draws(f.draws())
    try:
        ll = g.log_lik().reshape(-1, m.G * m.S)
    finally:
        g.close()
    a = P.log_ratios(*f.log_ratios())
    yield m, f, d, ll, a
    f.close()
    m.close()


def test_fit_matches_restatement(small_advi):
    m, f, d, ll, a = small_advi
    excl = np.isin(np.arange(m.G * m.S), EXCL)
    res = f.loo_approximate_posterior()
    ref = A.loo_columns(ll, a, excl)
    assert np.array_equal(res["excluded"].ravel(), excl) and res["n_draws"] == 1000
    for i, k in enumerate(L.FIELDS):
        _compare(res[k].ravel(), ref[:, i], 1e-12, k)
    assert np.all(np.isfinite(ref[:, 0]))
    est = L.estimates(ref, excl)
    for k in ("elpd_loo", "p_loo", "looic"):
        assert np.allclose(res["estimates"][k], est[k], rtol=1e-12, atol=0), k
    # the excluded cells: no effective parameters, and the k-hat of the approximation itself
    overall = f.psis(cols=[], overall=True)["khat"][-1]
    assert np.all(res["p_loo"].ravel()[excl] == 0)
    assert np.all(np.abs(res["khat"].ravel()[excl] - overall) <= 1e-12 * max(1.0, abs(overall)))
    assert res["khat_approximation"] == overall
    # the correction matters on this fit: plain PSIS-LOO of the same draws is another number
    assert np.max(np.abs(L.loo_columns(ll, None, excl)[~excl, 0] - ref[~excl, 0])) > 1e-3
    # a gene subset in another order, and a second call: the same bits
    sub = np.array([7, 0, 29, 4])
    s, again = f.loo_approximate_posterior(sub), f.loo_approximate_posterior()
    for k in L.FIELDS:
        assert np.array_equal(s[k], res[k][sub], equal_nan=True), k
        assert np.array_equal(again[k], res[k], equal_nan=True), k


def test_gene_batches_of_the_fit_give_the_same_bits():
    """the gene table of the walk in batches of one gene (testing build: the bound is a test hook) against one batch"""
    from ppcseq_amd.synth import synth
    d = synth(30, 10, K=4, seed=5)
    with testing_library() as _lib:
        mt = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=np.array(EXCL, np.int32), device=0)
        try:
            ft = mt.fit_advi(output_samples=1000, iter=2000, seed=3)
            try:
                base, pbase = ft.loo_approximate_posterior(), ft.loo_predict_approximate_posterior(seed=SEED)
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * 1000 + 8)
                try:
                    got, pgot = ft.loo_approximate_posterior(), ft.loo_predict_approximate_posterior(seed=SEED)
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
            finally:
                ft.close()
        finally:
            mt.close()
    assert np.all(np.isfinite(base["elpd_loo"]))
    for k in L.FIELDS:
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    for k in R.FIELDS:
        assert np.array_equal(pgot[k], pbase[k], equal_nan=True), k


def test_kernel_on_designed_columns():
    with testing_library() as _lib:
        for name, ll, a, excl in cases.designed():
            got = _lib.testing_loo_approx(ll[:, None], a, [int(excl)])[0]
            ref = np.array(A.loo_point(ll, a, excl))
            _compare(got, ref, 1e-12, name)
        # several columns of one launch are the columns one by one
        cs = [c for c in cases.designed() if c[1].size == 1000]
        assert len(cs) >= 8
        a = cs[0][2]
        lls, ex = np.stack([c[1] for c in cs], axis=1), [int(c[3]) for c in cs]
        both = _lib.testing_loo_approx(lls, a, ex)
        for i, c in enumerate(cs):
            assert np.array_equal(both[i], _lib.testing_loo_approx(lls[:, i:i + 1], a, ex[i:i + 1])[0], equal_nan=True), c[0]
        # the end of the LDS path and beyond; the scratch in several batches gives the same bits as one batch
        for n in (4096, 4097, 9000):
            ll, a, _, _, excl = cases.long_columns(n)
            one = _lib.testing_loo_approx(ll, a, excl)
            ref = A.loo_columns(ll, a, excl)
            for i in range(4):
                _compare(one[:, i], ref[:, i], 1e-12, (n, i))
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)                  # two cells per batch: r, ll, lw each
            try:
                assert np.array_equal(_lib.testing_loo_approx(ll, a, excl), one, equal_nan=True), n
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)


def test_predictive_kernel_on_designed_columns():
    with testing_library() as _lib:
        for name, ll, a, x, y, excl, p_lo, p_hi in cases.predictive():
            ref = A.predict_point(ll, a, x, y, excl, p_lo, p_hi)
            got = _lib.testing_loo_predict_approx(ll[:, None], a, x[:, None], [y], [int(excl)], p_lo, p_hi)[0]
            print(name, got, [ref[k] for k in R.FIELDS])
            if name.endswith("p = 0 / 1"):                       # F = p by construction: v* is the end of the support either way
                assert R.check(got, ref, None, x, 1.0, p_lo, p_hi, name) == 0
            else:
                assert A.predict_check(got, ref, ll, a, x, excl, p_lo, p_hi, name) == 0, name
            khat = _lib.testing_loo_approx(ll[:, None], a, [int(excl)])[0, 3]
            assert got[5] == khat or (np.isnan(got[5]) and (np.isnan(khat) or (x == R.INVALID).any())), name
        for n in (4096, 4097, 9000):
            ll, a, x, y, excl = cases.long_columns(n)
            one = _lib.testing_loo_predict_approx(ll, a, x, y, excl)
            for i in range(ll.shape[1]):
                ref = A.predict_point(ll[:, i], a, x[:, i], y[i], bool(excl[i]))
                assert A.predict_check(one[i], ref, ll[:, i], a, x[:, i], bool(excl[i]), what=(n, i)) == 0
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * (2 * n + (n + 1) // 2) + 8)       # two cells per batch
            try:
                assert np.array_equal(_lib.testing_loo_predict_approx(ll, a, x, y, excl), one, equal_nan=True), n
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        with pytest.raises(_lib.PpcxError, match="p_lo"):
            _lib.testing_loo_predict_approx(np.zeros((30, 1)), np.zeros(30), np.ones((30, 1)), [1], p_lo=0.5, p_hi=0.5)


def test_predictive_fit_matches_restatement(small_advi):
    m, f, d, ll, a = small_advi
    K, S = m.K, m.S
    _, x = f.ppc(1.0, 0.025, 0.975, seed=SEED, return_counts_rng=True)   # [n, K, S]: the predictive counts of the checked genes
    res = f.loo_predict_approximate_posterior(np.arange(K), seed=SEED)
    loo = f.loo_approximate_posterior(np.arange(K))
    assert "r_eff" not in res and res["n_draws"] == 1000
    skipped = 0
    for g in range(K):
        for s in range(S):
            excl = g * S + s in EXCL
            assert bool(res["excluded"][g, s]) == excl
            ref = A.predict_point(ll[:, g * S + s], a, x[:, g, s], int(d["counts"][g, s]), excl)
            got = [res[k][g, s] for k in R.FIELDS]
            skipped += A.predict_check(got, ref, ll[:, g * S + s], a, x[:, g, s], excl, what=(g, s)) > 0
    print("cells skipped as borderline:", skipped)
    assert skipped <= K * S / 1000
    assert np.array_equal(res["khat"], loo["khat"], equal_nan=True)
    assert np.array_equal(res["y"], d["counts"][:K])
    assert np.array_equal(res["outside"], (res["y"] < res["lower"]) | (res["y"] > res["upper"]))
    assert np.all(np.isfinite(res["mean"])) and np.all(res["lower"] <= res["upper"]) and np.all(res["pit_lt"] <= res["pit_le"])
    # the truncation compensation scales the predictive draws only
    c = f.loo_predict_approximate_posterior(np.arange(K), seed=SEED, truncation_compensation=0.7352941)
    assert np.array_equal(c["khat"], res["khat"]) and not np.array_equal(c["upper"], res["upper"])


def test_refusals(small_advi):
    from ppcseq_amd import _lib
    m, f, d, ll, a = small_advi
    for bad in ([m.G], [-1]):
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            f.loo_approximate_posterior(bad)
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            f.loo_predict_approximate_posterior(bad)
    for lo, hi in ((-0.1, 0.9), (0.5, 0.5), (np.nan, 0.9)):
        with pytest.raises(_lib.PpcxError, match="p_lo"):
            f.loo_predict_approximate_posterior([0], p_lo=lo, p_hi=hi)
    for tc in (0.0, np.inf):
        with pytest.raises(_lib.PpcxError, match="truncation_compensation"):
            f.loo_predict_approximate_posterior([0], truncation_compensation=tc)
    nuts = m.fit_nuts(chains=2, iter=60, warmup=40, seed=1)
    given = m.fit_from_draws(f.draws())
    try:
        for fit in (nuts, given):
            for call in (fit.loo_approximate_posterior, fit.loo_predict_approximate_posterior):
                with pytest.raises(_lib.PpcxError, match="needs an ADVI fit"):
                    call()
    finally:
        nuts.close()
        given.close()
    # the NUTS entry points keep refusing an ADVI fit
    for call in (f.loo, f.loo_predict):
        with pytest.raises(_lib.PpcxError, match="NUTS"):
            call()


def test_identify_outliers_check_approximation_loo(bundled):
    from ppcseq_amd.inference import loo_warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=True,
              how_many_negative_controls=50, cores=1, seed=11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(df, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = identify_outliers(df, check_approximation_loo=True, check_approximation_loo_intervals=True, **kw)
    assert not [k for k in plain.attrs if k.startswith("approximation_loo")]
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    K, S = 3, 21
    expect = []
    for key in ("approximation_loo_discovery", "approximation_loo_test"):
        r = out.attrs[key]
        for k in L.FIELDS + ("excluded",):
            assert r[k].shape == (K, S), (key, k)
        assert np.all(np.isfinite(r["elpd_loo"])), key
        assert np.all(np.abs(r["khat"][r["excluded"]] - r["khat_approximation"]) <= 1e-12 * max(1.0, abs(r["khat_approximation"]))), key
        expect += loo_warnings(r["khat"], r["n_draws"])
    got = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning) and str(x.message).startswith("Some Pareto k")]
    assert got == expect
    for key in ("approximation_loo_intervals_discovery", "approximation_loo_intervals_test"):
        r = out.attrs[key]
        for k in R.FIELDS + ("excluded", "y", "outside"):
            assert r[k].shape == (K, S), (key, k)
        assert np.all(np.isfinite(r["mean"])) and np.all(r["lower"] <= r["upper"]), key
        assert np.array_equal(r["outside"], (r["y"] < r["lower"]) | (r["y"] > r["upper"])), key
    assert out.attrs["approximation_loo_discovery"]["excluded"].sum() == 0
    assert np.array_equal(out.attrs["approximation_loo_test"]["excluded"], out.attrs["approximation_loo_intervals_test"]["excluded"])
