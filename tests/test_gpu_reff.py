"""The relative efficiency per observed cell on the MI355X (include/ppcx.h ppcx_fit_relative_eff) and r_eff="auto": the kernel on
the columns of the CPU check and beyond the LDS path (testing build) against the numpy restatement (tests/reff_restate.py), a
fit's cells against the restatement on its exported log-likelihood, determinism, Fit.loo / Fit.loo_predict with "auto",
refusals and identify_outliers(loo_r_eff="auto")."""
import numpy as np
import pytest

from tests import reff_restate as E
from tests.gpu_fixtures import small_fit, testing_library  # noqa: F401
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

TOL = 1e-9                                       # tests/test_gpu_summary.py's bar for the ESS on the device


def _compare(got, ref, what):
    got, ref = np.asarray(got, float).ravel(), np.asarray(ref, float).ravel()
    fin = ~np.isnan(ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    print(what, "max relative error", err.max(initial=0.0), "cells", ref.size, "NaN", int((~fin).sum()))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert err.max(initial=0.0) <= TOL, (what, err.max())


def test_kernel_on_the_host_checks_columns():
    with testing_library() as _lib:
        by_shape = {}
        for name, ll in list(E.seeded_cases()) + [(n, x) for n, x, _ in E.rule_cases()]:
            by_shape.setdefault(ll.shape, []).append((name, ll))
        rng = np.random.default_rng(5)
        x = -3.0 + E.ar1(rng, 0.5, 4, 64, 0.7)
        by_shape[(4, 64)] += [("underflow", x - 2000.0), ("underflow shifted", x)]
        for (M, n), cases in by_shape.items():
            ll = np.stack([c.ravel() for _, c in cases], axis=1)               # [M n][cells], chain-major
            got = _lib.testing_relative_eff(ll, M)
            ref = np.array([E.relative_eff(c) for _, c in cases])
            _compare(got, ref, (M, n))
            names = [nm for nm, _ in cases]
            if "-inf" in names:
                assert np.isfinite(got[names.index("-inf")])
            if "underflow" in names:
                a, b = got[names.index("underflow")], got[names.index("underflow shifted")]
                assert np.isfinite(a) and abs(a - b) <= 1e-12 * abs(b), (a, b)


def test_kernel_beyond_the_lds_path_and_in_batches():
    with testing_library() as _lib:
        M, n = 2, 2100                                                         # 4 200 draws: the split values in global scratch
        rng = np.random.default_rng(8)
        cols = [-3.0 + E.ar1(rng, phi, M, n, 0.7) for phi in (0.0, 0.5, 0.9, -0.5, 0.3, 0.7, 0.95)]
        c = rng.normal(size=(M, n)); c[1, 2000] = np.nan; cols.append(c)
        c = rng.normal(size=(M, n)); c[0, 7] = -np.inf; cols.append(c)
        ll = np.stack([c.ravel() for c in cols], axis=1)
        one = _lib.testing_relative_eff(ll, M)
        _compare(one, [E.relative_eff(c) for c in cols], "global path")
        _lib.testing_set("loo_scratch_bytes", 2 * 8 * M * n + 8)              # two cells per batch
        try:
            assert np.array_equal(_lib.testing_relative_eff(ll, M), one, equal_nan=True)
        finally:
            _lib.testing_set("loo_scratch_bytes", 0)


def test_fit_matches_restatement_and_is_deterministic(small_fit):
    m, f, d = small_fit
    ll = f.log_lik()                                                           # [chains, n_keep, G, S]
    re = f.relative_eff()
    assert re.shape == (m.G, m.S)
    ref = np.array([[E.relative_eff(ll[:, :, g, s]) for s in range(m.S)] for g in range(m.G)])
    _compare(re, ref, "fit")
    assert np.all(np.isfinite(re)) and np.all(re > 0)                          # the excluded cells (3, 17) hold a value too
    sub = np.array([7, 0, 29, 4])
    assert np.array_equal(f.relative_eff(sub), re[sub])
    assert np.array_equal(f.relative_eff(), re)
    g = m.fit_from_draws(f.draws())
    try:
        assert np.array_equal(g.relative_eff(), re)
    finally:
        g.close()


def test_loo_with_auto(small_fit):
    from tests import loo_restate as L
    from ppcseq_amd._lib import LOO_PREDICT_FIELDS
    m, f, d = small_fit
    base, base_p = f.loo(), f.loo_predict(seed=4)
    assert "r_eff" not in base and "r_eff" not in base_p
    re = f.relative_eff()
    filled = np.where(np.isnan(re), 1.0, re)
    auto, given = f.loo(r_eff="auto"), f.loo(r_eff=filled)
    assert np.array_equal(auto["r_eff"], filled) and "r_eff" not in given
    for k in L.FIELDS:
        assert np.array_equal(auto[k], given[k], equal_nan=True), k
    assert repr(auto["estimates"]) == repr(given["estimates"])
    sub = np.array([5, 1])
    asub = f.loo(sub, r_eff="auto")
    assert np.array_equal(asub["r_eff"], filled[sub]) and np.array_equal(asub["khat"], auto["khat"][sub], equal_nan=True)
    auto_p, given_p = f.loo_predict(r_eff="auto", seed=4), f.loo_predict(r_eff=filled, seed=4)
    assert np.array_equal(auto_p["r_eff"], filled)
    for k in LOO_PREDICT_FIELDS:
        assert np.array_equal(auto_p[k], given_p[k], equal_nan=True), k
    assert np.array_equal(auto_p["khat"], auto["khat"], equal_nan=True)
    again, again_p = f.loo(), f.loo_predict(seed=4)                            # the default is what it was
    for k in L.FIELDS:
        assert np.array_equal(again[k], base[k], equal_nan=True), k
    for k in LOO_PREDICT_FIELDS:
        assert np.array_equal(again_p[k], base_p[k], equal_nan=True), k


def test_refusals(small_fit):
    from ppcseq_amd import _lib
    m, f, d = small_fit
    for bad in ([m.G], [-1]):
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            f.relative_eff(bad)
    for call in (f.loo, f.loo_predict):
        with pytest.raises(ValueError, match="r_eff"):
            call(r_eff="bogus")
    a = m.fit_advi(output_samples=100, iter=500, seed=1)
    try:
        with pytest.raises(_lib.PpcxError, match="NUTS"):
            a.relative_eff()
        with pytest.raises(_lib.PpcxError, match="NUTS"):
            a.loo(r_eff="auto")
    finally:
        a.close()


def test_identify_outliers_loo_r_eff(bundled):
    import warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11, check_loo=True)
    K, S = 3, 21
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(df, **kw)
        out = identify_outliers(df, loo_r_eff="auto", pass_fit=True, **kw)
    fits = [out.attrs["fit 1"], out.attrs["fit 2"]]
    try:
        for key in ("loo_discovery", "loo_test"):
            assert "r_eff" not in plain.attrs[key]
            r = out.attrs[key]["r_eff"]
            assert r.shape == (K, S) and np.all(np.isfinite(r)) and np.all(r > 0), key
        # the second fit's model still holds the cells its pass excluded: the pass's numbers, recomputed
        f2 = fits[1]
        re = f2.relative_eff(np.arange(K))
        filled = np.where(np.isnan(re), 1.0, re)
        direct = f2.loo(np.arange(K), r_eff=filled)
        got = out.attrs["loo_test"]
        assert np.array_equal(got["r_eff"], filled)
        assert np.array_equal(got["khat"], direct["khat"], equal_nan=True)
        assert np.array_equal(got["elpd_loo"], direct["elpd_loo"], equal_nan=True)
    finally:
        for f in fits:
            f.close()
    for col in plain.columns:
        if col != "sample_wise_data":
            assert plain[col].tolist() == out[col].tolist(), col
    for a, b in zip(plain["sample_wise_data"], out["sample_wise_data"]):
        assert a.equals(b)
