"""The exact posterior-predictive tail probabilities and interval per cell on the MI355X (include/ppcx.h ppcx_fit_ppc_exact):
the device's negative-binomial tails against the CPU build at the edge points (testing build), the kernel on designed columns
against ppc_exact_cell_host, NUTS / ADVI / fit_from_draws fits of the bundled 53 x 21 case against the scipy restatement
(tests/ppc_exact_restate.py) fed with Fit.columns of the same draws, gene subsets, excluded cells, Fit.ppc's sampled interval
inside the exact one, refusals and identify_outliers(exact_intervals=True).

Tolerances: the tails at ppc_exact_restate.TAILS_BOUND (tests/test_nbcdf_host.py); the kernel against the CPU build: the integer
fields (lower, upper, y, excluded, outside) equal, mean, sd, p_le, p_ge 1e-12 relative (the sums run in another order, and the
device's exp / log are not libm's); against the restatement: ppc_exact_restate.check."""
import numpy as np
import pytest

from tests import ppc_exact_restate as R
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


def _against_host(got, ref, what):
    if np.isnan(ref[0]):
        assert np.array_equal(got, ref, equal_nan=True), (what, got, ref)
        return
    for i in (4, 5, 6, 7, 8):
        assert got[i] == ref[i], (what, R.FIELDS[i], got, ref)
    for i in (0, 1, 2, 3):
        assert abs(got[i] - ref[i]) <= 1e-12 * abs(ref[i]), (what, R.FIELDS[i], got[i], ref[i])


def test_device_tails_match_the_cpu_build(host):
    y, mu, phi = R.tails_points()
    eta = np.log(mu)
    le, ge, _ = R.host_tails(host, y, eta, phi)
    with testing_library() as _lib:
        dle, dge = _lib.testing_eval_math("nb2_tails", eta, phi, y)
        bad = _lib.testing_eval_math("nb2_tails", [np.nan, 1.0, 1.0, np.inf], [1.0, 0.0, np.inf, 1.0], [3, 3, 3, 3])
    err, ab = R.tails_errors(dle, dge, le, ge)
    print("largest error of the device against the CPU build", err.max(), "absolute", ab.max())
    assert not np.isnan(dle).any() and not np.isnan(dge).any()
    assert err.max() <= R.TAILS_BOUND and ab.max() <= R.TAILS_ABS
    assert np.all(dge[y == 0] == 1.0)
    assert np.isnan(bad[0]).all() and np.isnan(bad[1]).all()


def test_kernel_on_designed_columns(host):
    with testing_library() as _lib:
        for c in R.designed():
            kw = dict(excluded=c["excluded"], tc=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])
            ref, _ = R.host_cell(host, c["eta"], c["sg"], c["y"], **kw)
            got = _lib.testing_ppc_exact(c["eta"][:, None], c["sg"][:, None], [c["y"]], [int(c["excluded"])], c["tc"], c["p_lo"],
                                         c["p_hi"], raw=True)[0]
            _against_host(got, ref, c["name"])
        # the ends of the workgroup's stride, the LDS / scratch hand-over, and the scratch in batches of two cells
        for n in (1, 63, 64, 65, 4096, 4097, 9000):
            eta, sg, y = R.long_columns(n)
            one = _lib.testing_ppc_exact(eta, sg, y, truncation_compensation=R.TC, p_lo=R.P2, p_hi=1 - R.P2, raw=True)
            for i in range(eta.shape[1]):
                ref, _ = R.host_cell(host, eta[:, i], sg[:, i], y[i], tc=R.TC, p_lo=R.P2, p_hi=1 - R.P2)
                _against_host(one[i], ref, (n, i))
                alone = _lib.testing_ppc_exact(eta[:, i:i + 1], sg[:, i:i + 1], y[i:i + 1], truncation_compensation=R.TC, p_lo=R.P2,
                                               p_hi=1 - R.P2, raw=True)
                assert np.array_equal(alone[0], one[i]), (n, i)
            if n == 9000:
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * 2 * n + 8)             # two cells per batch
                try:
                    again = _lib.testing_ppc_exact(eta, sg, y, truncation_compensation=R.TC, p_lo=R.P2, p_hi=1 - R.P2, raw=True)
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
                assert np.array_equal(again, one), n
        d = _lib.testing_ppc_exact(np.full((30, 2), 2.0), np.zeros((30, 2)), [0, 2580228])
        assert d["lower"].dtype == np.int64 and d["outside"].dtype == bool and d["outside"].tolist() == [False, True]
        for lo, hi in ((0.0, 0.9), (0.5, 0.5), (0.6, 0.4), (0.1, 1.0), (np.nan, 0.9)):
            with pytest.raises(_lib.PpcxError, match="p_lo"):
                _lib.testing_ppc_exact(np.zeros((30, 1)), np.zeros((30, 1)), [1], p_lo=lo, p_hi=hi)


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X, expo, K, device=0)
    nuts = m.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    given = m.fit_from_draws(nuts.draws())
    yield dict(m=m, counts=counts, X=X, expo=expo, K=K, nuts=nuts, advi=advi, given=given)
    for f in (nuts, advi, given):
        f.close()
    m.close()


def _columns(f, fit):
    """eta [n, K, S] and sigma_raw [n, K] of the checked genes from Fit.columns (C = 2)"""
    G, K = f["m"].G, f["K"]
    a0 = fit.columns(3 + np.arange(K)).reshape(-1, K)
    a1 = fit.columns(3 + G + np.arange(K)).reshape(-1, K)
    sg = fit.columns(3 + G + K + np.arange(K)).reshape(-1, K)
    X = f["X"]
    eta = f["expo"][None, None, :] + a0[:, :, None] * X[None, None, :, 0] + a1[:, :, None] * X[None, None, :, 1]
    return eta, sg


@pytest.mark.parametrize("kind", ["nuts", "advi", "given"])
def test_fit_matches_restatement(fits, kind):
    f = fits
    fit = f[kind]
    K, S = f["K"], f["m"].S
    eta, sg = _columns(f, fit)
    res = fit.ppc_exact(p_lo=R.P2, p_hi=1 - R.P2, truncation_compensation=R.TC)
    assert res["n_draws"] == eta.shape[0] and res["genes"].tolist() == list(range(K))
    used = cells = 0
    for g in range(K):
        for s in range(g, S, 3):                                         # a third of the cells: scipy's search is the slow part
            ref = R.point(eta[:, g, s], sg[:, g], int(f["counts"][g, s]), tc=R.TC, p_lo=R.P2, p_hi=1 - R.P2)
            got = [float(res[k][g, s]) for k in R.FIELDS]
            used += R.check(got, ref, (kind, g, s))
            cells += 1
    assert used <= 0.02 * cells
    assert np.array_equal(res["y"], f["counts"][:K]) and not res["excluded"].any()
    assert np.array_equal(res["outside"], (res["y"] < res["lower"]) | (res["y"] > res["upper"]))
    if kind == "given":                                                  # the same draws: the same bits as the NUTS fit
        a = f["nuts"].ppc_exact(p_lo=R.P2, p_hi=1 - R.P2, truncation_compensation=R.TC)
        for k in R.FIELDS:
            assert np.array_equal(a[k], res[k], equal_nan=True), k


def test_subsets_and_excluded_cells(fits):
    f = fits
    fit, m = f["nuts"], f["m"]
    full = fit.ppc_exact()
    for sub in ([1], [2, 0], [2, 1, 0, 1]):
        r = fit.ppc_exact(sub)
        for k in R.FIELDS:
            assert np.array_equal(r[k], full[k][sub], equal_nan=True), (sub, k)
    S = m.S
    m.set_exclusions(np.array([0 * S + 3, 2 * S + 20], np.int32))
    try:
        ex = fit.ppc_exact()
    finally:
        m.set_exclusions(np.zeros(0, np.int32))
    assert ex["excluded"].sum() == 2 and ex["excluded"][0, 3] and ex["excluded"][2, 20]
    for k in R.FIELDS:
        if k != "excluded":
            assert np.array_equal(ex[k], full[k], equal_nan=True), k


def test_sampled_interval_lies_inside_the_exact_one(fits):
    """Fit.ppc's lower / upper are type-7 quantiles of n sampled counts, one per kept draw. A sample quantile at probability p
    of n draws is the exact quantile at a probability within 5 sqrt(p (1 - p) / n) of p (5 binomial standard errors of the
    empirical cdf at that point), so:  Q(p - 5 se) - 1 <= sampled <= Q(p + 5 se)  (- 1: type 7 interpolates downwards from an
    order statistic to the one below it, which is itself >= Q(p - 5 se) only up to that order statistic's own step)."""
    fit = fits["nuts"]
    n = fit.chains * fit.n_keep
    p = 0.025
    se = np.sqrt(p * (1 - p) / n)
    ci = fit.ppc(1.0, p, 1 - p, seed=5)
    eps = 1e-9
    lo = fit.ppc_exact(p_lo=max(p - 5 * se, eps), p_hi=p + 5 * se)
    hi = fit.ppc_exact(p_lo=1 - p - 5 * se, p_hi=min(1 - p + 5 * se, 1 - eps))
    assert np.all(ci[..., 2] >= lo["lower"] - 1) and np.all(ci[..., 2] <= lo["upper"])
    assert np.all(ci[..., 3] >= hi["lower"] - 1) and np.all(ci[..., 3] <= hi["upper"])
    ex = fit.ppc_exact(p_lo=p, p_hi=1 - p)
    assert np.all(np.abs(ci[..., 0] - ex["mean"]) <= 5 * ex["sd"] / np.sqrt(n))


def test_refusals(fits):
    from ppcseq_amd import _lib
    fit, K = fits["nuts"], fits["K"]
    for bad in ([K], [-1], [0, 52]):
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            fit.ppc_exact(bad)
    for lo, hi in ((0.0, 0.9), (-0.1, 0.9), (0.5, 0.5), (0.6, 0.4), (0.1, 1.0), (np.nan, 0.9)):
        with pytest.raises(_lib.PpcxError, match="p_lo"):
            fit.ppc_exact([0], p_lo=lo, p_hi=hi)
    for tc in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_lib.PpcxError, match="truncation_compensation"):
            fit.ppc_exact([0], truncation_compensation=tc)


def test_identify_outliers_exact_intervals(bundled):
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11)
    plain = identify_outliers(df, **kw)
    out = identify_outliers(df, exact_intervals=True, **kw)
    assert "exact_intervals_test" not in plain.attrs
    assert sorted(set(out.attrs) - set(plain.attrs)) == ["exact_intervals_discovery", "exact_intervals_test"]
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    K, S = 3, 21
    for key in ("exact_intervals_discovery", "exact_intervals_test"):
        r = out.attrs[key]
        for k in R.FIELDS:
            assert r[k].shape == (K, S), (key, k)
        assert np.all(np.isfinite(r["mean"])) and np.all(r["lower"] <= r["upper"]) and np.all(r["lower"] >= 0), key
    assert out.attrs["exact_intervals_discovery"]["excluded"].sum() == 0
    assert out.attrs["exact_intervals_test"]["excluded"].sum() >= 1        # the discovery pass's outliers are held out of pass 2
