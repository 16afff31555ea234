"""The two rows that the exact leave-one-out intervals add to inference.CHECKS, on the host, beside
tests/test_pass_checks_host.py: behind a recording stand-in for _lib.Model / Fit, exact_loo_intervals (NUTS, pooled chains
allowed) and exact_approximation_loo_intervals (ADVI) produce exactly one read of the fit with the pass's keywords, loo_r_eff is
accepted with exact_loo_intervals alone, and the wrong kind of pass is refused with the option's name first."""
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of the new options"""
    poor = standin.cells(khat=0.9)
    return standin.install(monkeypatch, dict(loo_predict_exact=poor, loo_predict_exact_approximate_posterior=poor))


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
