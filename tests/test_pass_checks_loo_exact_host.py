"""The two rows that the exact leave-one-out intervals add to inference.CHECKS, on the host, beside
tests/test_pass_checks_host.py: behind a recording stand-in for _lib.Model / Fit, exact_loo_intervals (NUTS, pooled chains
allowed) and exact_approximation_loo_intervals (ADVI) produce exactly one read of the fit with the pass's keywords, loo_r_eff is
accepted with exact_loo_intervals alone, and the wrong kind of pass is refused with the option's name first."""
import warnings

import numpy as np
import pytest

G, S, K = 6, 4, 2
COUNTS = np.random.default_rng(0).integers(5, 50, size=(G, S)).astype(np.int32)
X = np.stack([np.ones(S), np.array([0.0, 1.0, 0.0, 1.0])], axis=1)
PASS = dict(how_many_posterior_draws=300, cores=3, seed=7, launch=(8, 0), adj_prob_theshold=0.05, truncation_compensation=0.7)


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of the new options"""
    from ppcseq_amd import _lib
    log = []

    class Fit:
        def __init__(self, model, chains, n_keep):
            self.model, self.chains, self.n_keep, self.iter = model, chains, n_keep, n_keep + 150

        def ppc(self, *a, **kw):
            ci = np.zeros((self.model.K, self.model.S, 4))
            ci[..., 0], ci[..., 1], ci[..., 3] = 3.0, 1.0, 2.0
            return ci

        def columns(self, cols):
            return np.ones((self.chains, self.n_keep, len(cols)))

        def loo_predict_exact(self, genes, **kw):
            log.append(("loo_predict_exact", np.asarray(genes).tolist(), kw))
            return dict(khat=np.full((len(genes), self.model.S), 0.9))

        def loo_predict_exact_approximate_posterior(self, genes, **kw):
            log.append(("loo_predict_exact_approximate_posterior", np.asarray(genes).tolist(), kw))
            return dict(khat=np.full((len(genes), self.model.S), 0.9))

        def diagnostics(self):
            return dict(divergent=np.zeros((self.chains, self.iter), np.int32), treedepth=np.full((self.chains, self.iter), 3))

        def advi_info(self):
            return dict(iterations=1, converged=True, elbo=0.0, eta=1.0)

        def close(self):
            pass

    class Model:
        def __init__(self, counts, X, exposure_rate, K, **kw):
            self.G, self.S = np.shape(counts)
            self.K = int(K)

        def set_exclusions(self, excl):
            pass

        def set_launch(self, *a):
            pass

        def fit_nuts(self, **kw):
            return Fit(self, kw["chains"], kw["iter"] - kw["warmup"])

        def fit_advi(self, **kw):
            return Fit(self, 1, kw["output_samples"])

        def fit_from_draws(self, draws):
            log.append(("fit_from_draws",))
            return Fit(self, draws.shape[0], draws.shape[1])

        def close(self):
            pass

    monkeypatch.setattr(_lib, "Model", Model)
    monkeypatch.setattr(_lib, "device_memory", lambda device=0: (1 << 40, 1 << 40))
    return log


def _pass(**kw):
    from ppcseq_amd.inference import do_inference
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = do_inference(COUNTS, X, np.zeros(S), K, **PASS, **kw)
    return res, w


def test_exact_loo_intervals_reads_the_fit(rec):
    interval = dict(p_lo=0.05, p_hi=0.95, truncation_compensation=0.7)
    res, w = _pass(exact_loo_intervals=True)
    assert rec == [("loo_predict_exact", [0, 1], dict(r_eff=None, **interval))]
    assert res.exact_loo_intervals is not None and res.exact_approximation_loo_intervals is None and res.loo_intervals is None
    assert not w                                                   # the poor k-hats are check_loo's to report
    del rec[:]
    res, _ = _pass(exact_loo_intervals=True, loo_r_eff="auto")       # loo_r_eff with exact_loo_intervals alone
    assert rec == [("loo_predict_exact", [0, 1], dict(r_eff="auto", **interval))]
    del rec[:]
    res, _ = _pass(exact_loo_intervals=True, devices=[0, 0])         # over the pooled chains
    assert rec == [("fit_from_draws",), ("loo_predict_exact", [0, 1], dict(r_eff=None, **interval))]
    assert res.exact_loo_intervals is not None
    del rec[:]
    res, w = _pass(exact_approximation_loo_intervals=True, approximate_posterior_inference=True)
    assert rec == [("loo_predict_exact_approximate_posterior", [0, 1], interval)]
    assert res.exact_approximation_loo_intervals is not None and res.exact_loo_intervals is None and not w
    del rec[:]
    res, _ = _pass()
    assert rec == [] and res.exact_loo_intervals is None and res.exact_approximation_loo_intervals is None


def test_exact_loo_intervals_refusals(rec):
    import pandas as pd
    from ppcseq_amd.inference import CHECK_OPTIONS, do_inference
    from ppcseq_amd.methods import identify_outliers
    assert {"exact_loo_intervals", "exact_approximation_loo_intervals"} <= set(CHECK_OPTIONS)
    with pytest.raises(ValueError, match="^exact_loo_intervals needs a NUTS pass.*exact_approximation_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, exact_loo_intervals=True, **PASS)
    with pytest.raises(ValueError, match="^exact_approximation_loo_intervals needs an ADVI pass.*are exact_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_approximation_loo_intervals=True, **PASS)
    with pytest.raises(ValueError, match="^loo_r_eff needs check_loo, check_loo_intervals or exact_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, loo_r_eff="auto", **PASS)
    with pytest.raises(ValueError, match="^loo_r_eff needs"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, loo_r_eff="auto",
                     exact_approximation_loo_intervals=True, **PASS)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    kw = dict(transcript="symbol", abundance="value")
    with pytest.raises(ValueError, match="^exact_loo_intervals needs a NUTS pass"):
        identify_outliers(df, approximate_posterior_inference=True, exact_loo_intervals=True, **kw)
    with pytest.raises(ValueError, match="^exact_approximation_loo_intervals needs an ADVI pass"):
        identify_outliers(df, approximate_posterior_inference=False, exact_approximation_loo_intervals=True, **kw)
    with pytest.raises(ValueError, match="^exact_loo_intervals is not available for passes over several ranks"):
        identify_outliers(df, approximate_posterior_inference=False, exact_loo_intervals=True, _pass=object(), **kw)
    assert rec == []


def test_identify_outliers_reads_both_passes_at_their_own_settings(rec):
    """each pass at its own interval probability (0.05, then 0.005 = 1 % / 4 samples x 2) and truncation compensation; the
    results go to attrs["<field>_discovery"] and ["<field>_test"]"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3)
    settings = [dict(p_lo=0.05, p_hi=0.95, truncation_compensation=1.0), dict(p_lo=0.005, p_hi=0.995, truncation_compensation=0.7352941)]
    for option, advi, method, extra in (("exact_loo_intervals", False, "loo_predict_exact", dict(r_eff="auto")),
                                        ("exact_approximation_loo_intervals", True, "loo_predict_exact_approximate_posterior", {})):
        del rec[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plain = identify_outliers(data, approximate_posterior_inference=advi, **kw)
            assert rec == []
            out = identify_outliers(data, approximate_posterior_inference=advi, **{option: True}, **kw,
                                    **({"loo_r_eff": "auto"} if extra else {}))
        assert [(c[0], c[1]) for c in rec] == [(method, [0, 1])] * 2
        for c, s in zip(rec, settings):
            assert set(c[2]) == set(s) | set(extra) and all(c[2][k] == v for k, v in extra.items())
            assert all(abs(c[2][k] - v) <= 1e-12 for k, v in s.items()), (c[2], s)
        assert sorted(set(out.attrs) - set(plain.attrs)) == [option + "_discovery", option + "_test"]
        for col in plain.columns:
            assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
