"""The exact leave-one-out predictive tail probabilities and interval per cell on the MI355X (include/ppcx.h
ppcx_fit_loo_predict_exact, ppcx_fit_loo_predict_exact_approx): the kernel on the designed columns and at the lengths where the
workgroup's stride and the LDS / scratch hand-over can go wrong (testing build) against the CPU build of its header, NUTS and
ADVI fits of the bundled 53 x 21 case with two excluded cells against the scipy restatement (tests/loo_exact_restate.py) fed
with Fit.columns and Fit.log_lik of the same draws, k-hat against Fit.loo_predict bit for bit, excluded cells against
Fit.ppc_exact bit for bit, determinism, refusals and identify_outliers(exact_loo_intervals / exact_approximation_loo_intervals).

Tolerances: the kernel against the CPU build: the integer fields (lower, upper, y, excluded, outside) and a k-hat that is NaN or
Inf equal, mean, sd, p_le, p_ge and a finite k-hat 1e-12 relative (the sums run in another order, and the device's exp / log
are not libm's: test_gpu_ppc_exact._against_host's rule); against the restatement: loo_exact_restate.check, the one-count
allowance for at most 2 % of the interval ends."""
import numpy as np
import pytest

from tests import loo_exact_cases as cases
from tests import loo_exact_restate as R
from tests import psis_restate as P
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu
KEYS = R.FIELDS + ("pit_lt", "pit_le")


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


def _against_host(got, ref, what, worst=None):
    if np.isnan(ref[0]):
        assert np.array_equal(got, ref, equal_nan=True), (what, got, ref)
        return
    for i in (4, 5, 6, 7, 8):
        assert got[i] == ref[i], (what, R.FIELDS[i], got, ref)
    for i in (0, 1, 2, 3, 9):
        if not np.isfinite(ref[i]):
            assert np.array_equal(got[i], ref[i], equal_nan=True), (what, R.FIELDS[i], got[i], ref[i])
            continue
        err = abs(got[i] - ref[i]) / abs(ref[i]) if ref[i] != 0 else abs(got[i])
        if worst is not None:
            worst[0] = max(worst[0], err)
        assert err <= 1e-12, (what, R.FIELDS[i], got[i], ref[i])


def _hook(_lib, ll, eta, sg, y, **kw):
    return _lib.testing_loo_exact(ll, eta, sg, y, raw=True, **kw)


def test_kernel_on_designed_columns(host):
    worst = [0.0]
    with testing_library() as _lib:
        for c in cases.designed():
            kw = dict(excluded=[int(c["excluded"])], log_ratio=c["lr"], truncation_compensation=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])
            if c["lr"] is None:
                kw["r_eff"] = [c["r_eff"]]
            if c["refused"]:
                with pytest.raises(_lib.PpcxError, match="p_lo"):
                    _hook(_lib, c["ll"][:, None], c["eta"][:, None], c["sg"][:, None], [c["y"]], **kw)
                continue
            ref, _ = R.host_cell(host, c["ll"], c["eta"], c["sg"], c["y"], log_ratio=c["lr"], excluded=c["excluded"], r_eff=c["r_eff"],
                                 tc=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])
            got = _hook(_lib, c["ll"][:, None], c["eta"][:, None], c["sg"][:, None], [c["y"]], **kw)[0]
            _against_host(got, ref, c["name"], worst)
        print("largest relative error of the device against the CPU build", worst[0])
        d = _lib.testing_loo_exact(np.full((30, 2), -2.0), np.full((30, 2), 2.0), np.zeros((30, 2)), [0, 2580228])
        assert d["lower"].dtype == np.int64 and d["outside"].dtype == bool and d["outside"].tolist() == [False, True]
        assert np.array_equal(d["pit_le"], d["p_le"]) and np.array_equal(d["pit_lt"], 1.0 - d["p_ge"]) and np.all(d["khat"] == np.inf)
        for lo, hi in ((0.0, 0.9), (0.5, 0.5), (0.6, 0.4), (0.1, 1.0), (np.nan, 0.9)):
            with pytest.raises(_lib.PpcxError, match="p_lo"):
                _lib.testing_loo_exact(np.zeros((30, 1)), np.zeros((30, 1)), np.zeros((30, 1)), [1], p_lo=lo, p_hi=hi)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4096, 4097, 9000])
def test_kernel_lengths(host, n):
    """the ends of the workgroup's stride, the LDS / scratch hand-over, and the scratch in batches of two cells; NUTS weights
    with r_eff and an excluded cell, then the ADVI weights"""
    with testing_library() as _lib:
        ll, eta, sg, y, excl, r_eff, lr = cases.long_columns(n)
        kw = dict(truncation_compensation=R.TC, p_lo=R.P2, p_hi=1 - R.P2)
        for form in (dict(r_eff=r_eff), dict(log_ratio=lr)):
            one = _hook(_lib, ll, eta, sg, y, excluded=excl, **form, **kw)
            for i in range(ll.shape[1]):
                ref, _ = R.host_cell(host, ll[:, i], eta[:, i], sg[:, i], y[i], log_ratio=form.get("log_ratio"), excluded=bool(excl[i]),
                                     r_eff=r_eff[i], tc=R.TC, p_lo=R.P2, p_hi=1 - R.P2)
                _against_host(one[i], ref, (n, i, list(form)))
                alone_form = dict(form) if "log_ratio" in form else dict(r_eff=r_eff[i:i + 1])
                alone = _hook(_lib, ll[:, i:i + 1], eta[:, i:i + 1], sg[:, i:i + 1], y[i:i + 1], excluded=excl[i:i + 1], **alone_form, **kw)
                assert np.array_equal(alone[0], one[i], equal_nan=True), (n, i, list(form))
            if n == 9000:
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)             # two cells per batch
                try:
                    again = _hook(_lib, ll, eta, sg, y, excluded=excl, **form, **kw)
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
                assert np.array_equal(again, one, equal_nan=True), list(form)


EXCL = (0 * 21 + 3, 2 * 21 + 20)                     # the two cells the model holds out


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X, expo, K, excl=np.array(EXCL, np.int32), device=0)
    nuts = m.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    given = m.fit_from_draws(nuts.draws())
    yield dict(m=m, counts=counts, X=X, expo=expo, K=K, nuts=nuts, advi=advi, given=given)
    for f in (nuts, advi, given):
        f.close()
    m.close()


def _columns(f, fit):
    """eta [n, K, S], sigma_raw [n, K] (Fit.columns, C = 2) and ll [n, K, S] of the checked genes (Fit.log_lik; of an ADVI fit
    through a fit that holds the same draws)"""
    G, K = f["m"].G, f["K"]
    a0 = fit.columns(3 + np.arange(K)).reshape(-1, K)
    a1 = fit.columns(3 + G + np.arange(K)).reshape(-1, K)
    sg = fit.columns(3 + G + K + np.arange(K)).reshape(-1, K)
    X = f["X"]
    eta = f["expo"][None, None, :] + a0[:, :, None] * X[None, None, :, 0] + a1[:, :, None] * X[None, None, :, 1]
    holder = fit if fit is not f["advi"] else f["m"].fit_from_draws(fit.draws())
    try:
        ll = holder.log_lik(np.arange(K)).reshape(-1, K, f["m"].S)
    finally:
        if holder is not fit:
            holder.close()
    return eta, sg, ll


def _fit_against_restatement(f, res, eta, sg, ll, lr, r_eff, what):
    K, S = f["K"], f["m"].S
    used = ends = 0
    for g in range(K):
        for s in range(S):
            excl = g * S + s in EXCL
            assert bool(res["excluded"][g, s]) == excl
            ref = R.point(ll[:, g, s], eta[:, g, s], sg[:, g], int(f["counts"][g, s]), log_ratio=lr, excluded=excl,
                          r_eff=1.0 if r_eff is None else r_eff[g, s], tc=R.TC, p_lo=R.P2, p_hi=1 - R.P2)
            used += R.check([float(res[k][g, s]) for k in R.FIELDS], ref, (what, g, s))
            ends += 2
    print(what, "interval ends", ends, "that used the one-count allowance", used)
    assert used <= 0.02 * ends
    assert np.array_equal(res["y"], f["counts"][:K]) and res["excluded"].sum() == 2
    assert np.array_equal(res["outside"], (res["y"] < res["lower"]) | (res["y"] > res["upper"]))
    assert np.array_equal(res["pit_le"], res["p_le"]) and np.array_equal(res["pit_lt"], 1.0 - res["p_ge"])


def test_nuts_fit_matches_restatement(fits):
    f = fits
    fit, K = f["nuts"], f["K"]
    eta, sg, ll = _columns(f, fit)
    kw = dict(p_lo=R.P2, p_hi=1 - R.P2, truncation_compensation=R.TC)
    for r_eff in (None, "auto"):
        res = fit.loo_predict_exact(r_eff=r_eff, **kw)
        assert res["n_draws"] == eta.shape[0] and res["genes"].tolist() == list(range(K))
        assert ("r_eff" in res) == (r_eff == "auto")
        _fit_against_restatement(f, res, eta, sg, ll, None, res.get("r_eff"), f"nuts r_eff={r_eff}")
        # k-hat is Fit.loo_predict's, bit for bit; the excluded cells are Fit.ppc_exact's
        lp = fit.loo_predict(np.arange(K), r_eff=r_eff, seed=3, **kw)
        assert np.array_equal(res["khat"], lp["khat"], equal_nan=True)
        assert np.isfinite(res["khat"][~res["excluded"]]).all() and np.isnan(res["khat"][res["excluded"]]).all()
        if r_eff == "auto":
            assert np.array_equal(res["r_eff"], lp["r_eff"])
        pe = fit.ppc_exact(**kw)
        for k in R.E.FIELDS:
            assert np.array_equal(res[k][res["excluded"]], pe[k][res["excluded"]], equal_nan=True), k
        assert not np.array_equal(res["mean"][~res["excluded"]], pe["mean"][~res["excluded"]])
    # the same draws loaded into a fit give the same bits (the pooled passes read such a fit)
    a, b = fit.loo_predict_exact(r_eff="auto", **kw), f["given"].loo_predict_exact(r_eff="auto", **kw)
    for k in KEYS + ("r_eff",):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_tails_hold_the_held_out_density(fits):
    """P(X <= y) + P(X >= y) - 1 = P(X = y): without truncation compensation p_le + p_ge - 1 is the cell's exp(elpd_loo)"""
    fit, K = fits["nuts"], fits["K"]
    for r_eff in (None, "auto"):
        res = fit.loo_predict_exact(r_eff=r_eff)
        loo = fit.loo(np.arange(K), r_eff=r_eff)
        d = np.abs(res["p_le"] + res["p_ge"] - 1.0 - np.exp(loo["elpd_loo"]))
        print("r_eff", r_eff, "largest difference", d.max())
        assert d.max() <= 2 * R.TAILS_ABS + 1e-12


def test_advi_fit_matches_restatement(fits):
    f = fits
    fit, K, S = f["advi"], f["K"], f["m"].S
    eta, sg, ll = _columns(f, fit)
    lp, lg = fit.log_ratios()
    kw = dict(p_lo=R.P2, p_hi=1 - R.P2, truncation_compensation=R.TC)
    res = fit.loo_predict_exact_approximate_posterior(**kw)
    assert "r_eff" not in res and res["n_draws"] == eta.shape[0]
    lr = P.log_ratios(lp, lg)
    _fit_against_restatement(f, res, eta, sg, ll, lr, None, "advi")
    ref = fit.loo_predict_approximate_posterior(np.arange(K), seed=3, **kw)
    assert np.array_equal(res["khat"], ref["khat"], equal_nan=True)
    overall = fit.loo_approximate_posterior(np.arange(K))["khat_approximation"]
    assert res["khat_approximation"] == overall
    assert np.all(res["khat"][res["excluded"]] == overall)            # an excluded cell carries the overall k-hat


def test_determinism_subsets_and_batches(fits):
    f = fits
    fit = f["nuts"]
    full = fit.loo_predict_exact(r_eff="auto")
    re = full["r_eff"]
    again = fit.loo_predict_exact(r_eff=re)
    for sub in ([1], [2, 0], [2, 1, 0]):
        r = fit.loo_predict_exact(sub, r_eff=re[sub])
        for k in KEYS:
            assert np.array_equal(r[k], full[k][sub], equal_nan=True), (sub, k)
            assert np.array_equal(again[k], full[k], equal_nan=True), k
    afull = f["advi"].loo_predict_exact_approximate_posterior()
    arev = f["advi"].loo_predict_exact_approximate_posterior([2, 1, 0])
    for k in KEYS:
        assert np.array_equal(arev[k], afull[k][::-1], equal_nan=True), k
    draws = fit.draws()
    n = draws.shape[0] * draws.shape[1]
    with testing_library() as _lib:
        mt = _lib.Model(f["counts"], f["X"], f["expo"], f["K"], excl=np.array(EXCL, np.int32), device=0)
        try:
            ft = mt.fit_from_draws(draws)
            try:
                got = []
                for genes_per_batch in (1, 2):                            # the gene table in batches of one or two genes
                    _lib.testing_set("loo_scratch_bytes", genes_per_batch * 8 * 3 * n + 8)
                    try:
                        got.append(ft.loo_predict_exact(r_eff=re))
                    finally:
                        _lib.testing_set("loo_scratch_bytes", 0)
            finally:
                ft.close()
        finally:
            mt.close()
    for g in got:
        for k in KEYS:
            assert np.array_equal(g[k], full[k], equal_nan=True), k


def test_refusals(fits):
    from ppcseq_amd import _lib
    f = fits
    nuts, advi, given, K, S = f["nuts"], f["advi"], f["given"], f["K"], f["m"].S
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_predict_exact needs the draws of a NUTS fit.*ppcx_fit_loo_predict_exact_approx"):
        advi.loo_predict_exact()
    for fit in (nuts, given):
        with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_predict_exact_approx needs an ADVI fit.*ppcx_fit_loo_predict_exact"):
            fit.loo_predict_exact_approximate_posterior()
    for call in (nuts.loo_predict_exact, advi.loo_predict_exact_approximate_posterior):
        for bad in ([K], [-1], [0, 52]):
            with pytest.raises(_lib.PpcxError, match="gene out of range"):
                call(bad)
        for lo, hi in ((0.0, 0.9), (-0.1, 0.9), (0.5, 0.5), (0.6, 0.4), (0.1, 1.0), (np.nan, 0.9)):
            with pytest.raises(_lib.PpcxError, match="p_lo"):
                call([0], p_lo=lo, p_hi=hi)
        for tc in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(_lib.PpcxError, match="truncation_compensation"):
                call([0], truncation_compensation=tc)
    with pytest.raises(ValueError):
        nuts.loo_predict_exact([0, 1], r_eff=np.ones((3, S)))             # an r_eff of the wrong shape
    with pytest.raises(ValueError):
        nuts.loo_predict_exact([0], r_eff="automatic")
    for r in (0.0, -1.0, np.nan, np.inf):
        re = np.ones((2, S)); re[1, 3] = r
        with pytest.raises(_lib.PpcxError, match="r_eff"):
            nuts.loo_predict_exact([0, 1], r_eff=re)


def _outliers_kw(advi):
    return dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
                do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=advi,
                approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11)


@pytest.mark.parametrize("option,advi", [("exact_loo_intervals", False), ("exact_approximation_loo_intervals", True)])
def test_identify_outliers_reports_the_exact_loo_intervals(bundled, option, advi):
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = _outliers_kw(advi)
    plain = identify_outliers(df, **kw)
    out = identify_outliers(df, **{option: True}, **kw)
    assert sorted(set(out.attrs) - set(plain.attrs)) == [option + "_discovery", option + "_test"]
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    K, S = 3, 21
    for key in (option + "_discovery", option + "_test"):
        r = out.attrs[key]
        for k in KEYS:
            assert r[k].shape == (K, S), (key, k)
        assert np.all(np.isfinite(r["mean"])) and np.all(r["lower"] <= r["upper"]) and np.all(r["lower"] >= 0), key
        assert ("khat_approximation" in r) == advi
    assert out.attrs[option + "_discovery"]["excluded"].sum() == 0
    assert out.attrs[option + "_test"]["excluded"].sum() >= 1            # the discovery pass's outliers are held out of pass 2
    # each pass's own probabilities and truncation compensation: tests/test_pass_checks_loo_exact_host.py holds the keywords
    with pytest.raises(ValueError, match="^" + option):
        identify_outliers(df, **{option: True}, **_outliers_kw(not advi))


def test_identify_outliers_over_pooled_chains(bundled):
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(_outliers_kw(False), cores=4, launch=(8, 0))
    plain = identify_outliers(df, devices=[0, 0], **kw)
    out = identify_outliers(df, devices=[0, 0], exact_loo_intervals=True, loo_r_eff="auto", **kw)
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    for key in ("exact_loo_intervals_discovery", "exact_loo_intervals_test"):
        r = out.attrs[key]
        assert r["mean"].shape == (3, 21) and r["r_eff"].shape == (3, 21) and np.all(np.isfinite(r["mean"])), key
        assert np.isfinite(r["khat"][~r["excluded"]]).all() and np.isnan(r["khat"][r["excluded"]]).all(), key
