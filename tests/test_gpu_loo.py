"""PSIS-LOO per observed cell on the MI355X (include/ppcx.h ppcx_fit_get_log_lik / ppcx_fit_loo): the log-likelihood against
scipy at the draws and mpmath at extreme cells, LOO against the numpy restatement (tests/loo_restate.py), the kernel on
designed columns (testing build), a brute-force leave-one-out refit, determinism, refusals and identify_outliers(check_loo)."""
import warnings

import numpy as np
import pytest

from tests import loo_restate as L
from tests.gpu_fixtures import small_fit, testing_library  # noqa: F401
from tests.test_gpu_psis import _bundled_frame, designs

pytestmark = pytest.mark.gpu


def _params(draws, G, C, K):
    """alpha [n, C, G] and sigma_raw [n, G] at each draw (oracle.independent.unpack)"""
    from oracle.independent import unpack
    n = draws.shape[0]
    alpha, sr = np.zeros((n, C, G)), np.zeros((n, G))
    for i in range(n):
        p = unpack(draws[i], G, C, K, 5.612671)
        alpha[i, 0] = p["intercept"]
        if C >= 2:
            alpha[i, 1, :K] = p["alpha1"]
        if C >= 3:
            alpha[i, 2:, :K] = p["alpha2"]
        sr[i] = p["sigma_raw"]
    return alpha, sr


def _reference_ll(counts, X, expo, draws, K):
    from scipy.special import gammaln
    G, S = counts.shape
    C = X.shape[1]
    alpha, sr = _params(draws, G, C, K)
    eta = np.einsum("sc,ncg->ngs", X, alpha) + expo[None, None, :]
    ref = L.log_lik(counts[None], eta, sr[:, :, None])
    y = counts[None].astype(float)
    phi = np.exp(-sr)[:, :, None]
    lw = np.logaddexp(0.0, eta + sr[:, :, None])
    scale = 1 + np.abs(y * eta) + (y + phi) * np.abs(lw) + gammaln(y + phi)
    return ref, scale


def _compare(got, ref, tol, what):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    assert err.max(initial=0.0) <= tol, (what, err.max())


def test_log_lik_matches_scipy(bundled):
    from ppcseq_amd import _lib
    for name, counts, X, expo, K, excl in designs(bundled):
        m = _lib.Model(counts, X, expo, K, excl=excl, device=0)
        try:
            f = m.fit_nuts(chains=2, iter=110, warmup=60, seed=4)
            try:
                ll = f.log_lik()
                G, S = counts.shape
                assert ll.shape == (2, 50, G, S), name
                dr = f.draws().reshape(-1, m.D)
                ref, scale = _reference_ll(np.asarray(counts), np.asarray(X, float).reshape(S, -1), np.asarray(expo), dr, K)
                err = np.abs(ll.reshape(-1, G, S) - ref) / scale
                assert err.max() <= 1e-12, (name, err.max())
                sub = np.array([G - 1, 0, 2])
                assert np.array_equal(f.log_lik(sub), ll[:, :, sub]), name
            finally:
                f.close()
        finally:
            m.close()


def test_log_lik_extreme_cells_against_mpmath():
    import mpmath
    from ppcseq_amd import _lib
    mpmath.mp.dps = 40
    counts = np.array([[0, 3, 2_600_000, 17], [0, 1, 9, 2_600_000], [5, 0, 40, 120]], np.int32)
    S = 4
    X = np.ones((S, 1))
    expo = np.array([0.0, -1.5, 2.0, 0.7])
    m = _lib.Model(counts, X, expo, 1, device=0)
    try:
        rows = []
        for icpt, sr in ((2.0, -9.5), (14.5, 10.5), (-3.0, 0.25), (14.0, -12.0), (0.1, 12.0)):
            u = np.zeros(m.D)
            u[3:6] = icpt
            u[3 + 3 + 1:3 + 3 + 1 + 3] = sr                     # sigma_raw of the three genes (C = 1, K = 1)
            rows.append(u)
        f = m.fit_from_draws(np.array(rows)[None])
        try:
            ll = f.log_lik()[0]
            for i, (icpt, sr) in enumerate(((2.0, -9.5), (14.5, 10.5), (-3.0, 0.25), (14.0, -12.0), (0.1, 12.0))):
                for g in range(3):
                    for s in range(S):
                        y = int(counts[g, s])
                        phi = mpmath.exp(-mpmath.mpf(sr))
                        mu = mpmath.exp(mpmath.mpf(expo[s]) + mpmath.mpf(icpt))
                        ref = (mpmath.loggamma(y + phi) - mpmath.loggamma(phi) - mpmath.loggamma(y + 1)
                               + y * (mpmath.log(mu) - mpmath.log(mu + phi)) + phi * (mpmath.log(phi) - mpmath.log(mu + phi)))
                        scale = 1 + abs(y * (expo[s] + icpt)) + float((y + phi) * abs(mpmath.log1p(mu / phi + 0)))
                        scale += float(abs(mpmath.loggamma(y + phi)))
                        assert abs(ll[i, g, s] - float(ref)) <= 1e-12 * scale, (icpt, sr, g, s, ll[i, g, s], float(ref))
        finally:
            f.close()
    finally:
        m.close()


def test_loo_matches_restatement(small_fit):
    m, f, d = small_fit
    ll = f.log_lik().reshape(-1, m.G * m.S)
    excl = np.zeros(m.G * m.S, bool)
    excl[[3, 17]] = True
    rng = np.random.default_rng(0)
    for r_eff in (None, rng.uniform(0.2, 1.5, size=(m.G, m.S))):
        res = f.loo(r_eff=r_eff)
        ref = L.loo_columns(ll, None if r_eff is None else r_eff.ravel(), excl)
        assert np.array_equal(res["excluded"].ravel(), excl)
        for i, k in enumerate(L.FIELDS):
            _compare(res[k].ravel(), ref[:, i], 1e-12, k)
        assert np.all(np.isnan(res["khat"].ravel()[excl])) and np.all(res["p_loo"].ravel()[excl] == 0)
        est = L.estimates(ref, excl)
        for k in ("elpd_loo", "p_loo", "looic"):
            assert np.allclose(res["estimates"][k], est[k], rtol=1e-12, atol=0), k


def test_kernel_on_designed_columns():
    with testing_library() as _lib:
        rng = np.random.default_rng(4)
        cols = [-L.P.normal_ratios(rng, s2, 3000) for s2 in (1.5, 3.0, 10.0)]
        cols.append(-np.log(L.P.gpd_sample(rng, 0.8, 3000)))
        cols.append(-rng.poisson(3.0, size=3000).astype(float))            # ties in the tail and at the cutoff
        c = rng.normal(size=3000); c[::9] = np.inf; cols.append(c)         # ll = +Inf takes no part
        c = rng.normal(size=3000); c[4] = -np.inf; cols.append(c)          # ll = -Inf: NaN
        c = rng.normal(size=3000); c[8] = np.nan; cols.append(c)
        cols.append(np.full(3000, -2.5))                                   # constant tail
        cols.append(rng.normal(-4.0, 0.5, size=3000))                      # excluded below
        ll = np.stack(cols, axis=1)
        excl = np.zeros(ll.shape[1], np.int32); excl[-1] = 1
        r_eff = rng.uniform(0.3, 2.0, size=ll.shape[1])
        for re in (None, r_eff):
            got = _lib.testing_loo(ll, excl, re)
            ref = L.loo_columns(ll, re, excl.astype(bool))
            for i in range(4):
                _compare(got[:, i], ref[:, i], 1e-12, ("designed", i))
        assert _lib.testing_loo(rng.normal(size=(20, 1)))[0, 3] == np.inf                  # M = 4
        # columns beyond the LDS path, and the scratch in several batches, give the same bits as one batch
        for n in (4096, 4097, 9000):
            ll = np.stack([-L.P.normal_ratios(rng, 2.5, n) for _ in range(7)], axis=1)
            one = _lib.testing_loo(ll)
            _compare(one[:, 0], L.loo_columns(ll)[:, 0], 1e-12, n)
            _compare(one[:, 3], L.loo_columns(ll)[:, 3], 1e-12, n)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * n + 8)                      # two columns per batch
            try:
                assert np.array_equal(_lib.testing_loo(ll), one, equal_nan=True), n
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)


def test_batches_of_the_fit_give_the_same_bits(small_fit):
    m, f, d = small_fit
    base, ll = f.loo(), f.log_lik()
    dr = f.draws()
    with testing_library() as _lib:
        mt = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=np.array([3, 17], np.int32), device=0)
        try:
            ft = mt.fit_from_draws(dr)
            try:
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * 1000 + 8)      # the gene table in batches of one or two genes
                try:
                    got, gll = ft.loo(), ft.log_lik()
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
            finally:
                ft.close()
        finally:
            mt.close()
    for k in L.FIELDS:
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    assert np.array_equal(gll, ll)


def test_gene_batches_over_scratch_batches_give_the_same_bits(small_fit):
    """The one walk of the per-cell statistics (for_gene_batches) where both of its bounds bind at once: a fit beyond the LDS
    path (4 x 1300 = 5200 draws: small_fit's draws repeated along the draw axis, with a jitter of 1e-3 so that no column is an
    exact copy), the gene table in fifteen batches of two genes and each batch's 20 cells in several scratch launches that
    reuse one allocation. Every statistic gives the bits of the unbounded call, and the unbounded LOO is the restatement's on
    the fit's own log-likelihood, at the bound of test_loo_matches_restatement."""
    m, f, d = small_fit
    own = L.loo_columns(f.log_lik().reshape(-1, m.G * m.S), None, np.isin(np.arange(m.G * m.S), [3, 17]))
    dr = np.tile(f.draws(), (1, 6, 1))[:, :1300]
    dr = dr + 1e-3 * np.sin(np.arange(dr.size, dtype=np.float64)).reshape(dr.shape)
    n, C = 4 * 1300, np.asarray(d["X"]).reshape(m.S, -1).shape[1]

    def calls(ft):
        return dict(loo=ft.loo(), mcse=ft.loo(mcse=True), predict=ft.loo_predict(), reff=dict(r_eff=ft.relative_eff()))

    with testing_library() as _lib:
        mt = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=np.array([3, 17], np.int32), device=0)
        try:
            ft = mt.fit_from_draws(dr)
            try:
                one, ll = calls(ft), ft.log_lik().reshape(n, m.G * m.S)
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * (C + 1) * n + 8)   # two genes per table batch
                try:
                    got = calls(ft)
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
            finally:
                ft.close()
        finally:
            mt.close()
    for what, res in one.items():
        for k, v in res.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(got[what][k], v, equal_nan=True), (what, k)
    ref = L.loo_columns(ll, None, one["loo"]["excluded"].ravel())
    for i, k in enumerate(L.FIELDS):
        _compare(one["loo"][k].ravel(), ref[:, i], 1e-12, k)
    nan_here, nan_own = np.isnan(ref[:, 0]).mean(), np.isnan(own[:, 0]).mean()
    print("NaN share of elpd_loo: jittered fit", nan_here, "small_fit", nan_own)
    assert nan_here <= nan_own


def test_determinism(small_fit):
    m, f, d = small_fit
    a, b = f.loo(), f.loo()
    sub = np.array([7, 0, 29, 4])
    s = f.loo(sub)
    dr = f.draws()
    g = m.fit_from_draws(dr)
    try:
        c = g.loo()
        assert np.array_equal(g.log_lik(), f.log_lik())
    finally:
        g.close()
    for k in L.FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(s[k], a[k][sub], equal_nan=True), k
        assert np.array_equal(c[k], a[k], equal_nan=True), k


def test_brute_force_leave_one_out():
    """PSIS-LOO of the full fit against the held-out density of refits without the cell. Tolerance: 5 Monte-Carlo standard
    errors of the difference, each from the draws (relative error of the mean of exp(ll) -- refit -- and of exp(-ll) -- the
    importance-sampling estimate), with the effective sample size taken as a quarter of the draws for autocorrelation."""
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(12, 8, K=2, seed=7)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 2, device=0)
    try:
        f = m.fit_nuts(chains=4, iter=1150, warmup=150, seed=2)
        try:
            res = f.loo()
            ll = f.log_lik().reshape(-1, m.G * m.S)
        finally:
            f.close()
        khat = res["khat"].ravel()
        cells = [int(c) for c in np.argsort(-res["p_loo"].ravel()) if khat[c] < 0.5][:3]
        n_eff = ll.shape[0] / 4
        for c in cells:
            m.set_exclusions(np.array([c], np.int32))
            r = m.fit_nuts(chains=4, iter=1150, warmup=150, seed=2)
            try:
                held = r.loo([c // m.S])
                llr = r.log_lik([c // m.S])[..., c % m.S].ravel()
            finally:
                r.close()
            assert held["excluded"].ravel()[c % m.S]
            e_ref = held["elpd_loo"].ravel()[c % m.S]
            wr = np.exp(llr - llr.max())
            wf = np.exp(-ll[:, c] + ll[:, c].min())
            se = np.sqrt((wr.std() / wr.mean()) ** 2 / n_eff + (wf.std() / wf.mean()) ** 2 / n_eff)
            e_psis = res["elpd_loo"].ravel()[c]
            assert abs(e_psis - e_ref) <= 5 * se, (c, e_psis, e_ref, se)
    finally:
        m.close()


def test_refusals(small_fit):
    from ppcseq_amd import _lib
    m, f, d = small_fit
    for bad in ([m.G], [-1]):
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            f.loo(bad)
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            f.log_lik(bad)
    for r in (0.0, -1.0, np.nan, np.inf):
        re = np.ones((2, m.S)); re[1, 3] = r
        with pytest.raises(_lib.PpcxError, match="r_eff"):
            f.loo([0, 1], r_eff=re)
    a = m.fit_advi(output_samples=100, iter=500, seed=1)
    try:
        for call in (a.loo, a.log_lik):
            with pytest.raises(_lib.PpcxError, match="NUTS"):
                call()
    finally:
        a.close()


def test_identify_outliers_check_loo(bundled):
    from ppcseq_amd.inference import loo_warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11)
    plain = identify_outliers(df, **kw)
    off = identify_outliers(df, check_loo=False, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = identify_outliers(df, check_loo=True, **kw)
    assert "loo_test" not in plain.attrs and "loo_test" not in off.attrs
    for col in plain.columns:
        a, b = plain[col].tolist(), off[col].tolist()
        assert repr(a) == repr(b), col
    K, S = 3, 21
    expect = []
    for key in ("loo_discovery", "loo_test"):
        r = out.attrs[key]
        for k in L.FIELDS:
            assert r[k].shape == (K, S), (key, k)
        assert np.all(np.isfinite(r["elpd_loo"])), key
        expect += loo_warnings(r["khat"], r["n_draws"])
    got = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning) and "Pareto k" in str(x.message)]
    assert got == expect
    assert out.attrs["loo_discovery"]["excluded"].sum() == 0
    assert out.attrs["loo_test"]["excluded"].sum() >= 1                # the discovery pass's outliers are held out
    assert out["tot_deleterious_outliers"].tolist() == plain["tot_deleterious_outliers"].tolist()
