"""The modifier that the exact leave-one-out predictive under moment-matched weights adds to inference.MODIFIERS, on the host,
beside tests/test_pass_checks_loo_mm_host.py: behind a recording stand-in for _lib.Model / Fit, exact_loo_moment_match turns
exact_loo_intervals' one read of the fit into Fit.loo_predict_exact_moment_match with the pass's r_eff, interval probabilities
and truncation compensation (pooled chains allowed), a call without the modifier carries exactly the keywords it carried
before, loo_moment_match keeps affecting check_loo only, and the modifier is refused without exact_loo_intervals."""
import inspect
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass

INTERVAL = dict(p_lo=0.05, p_hi=1 - 0.05, truncation_compensation=0.7)      # the pass's adj_prob_theshold and compensation


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of exact_loo_intervals and check_loo"""
    good = standin.cells(khat=0.3)
    return standin.install(monkeypatch, dict(loo=good, loo_moment_match=good, loo_predict_exact=good,
                                             loo_predict_exact_moment_match=standin.cells(khat=0.3, khat_before=0.9)))


def _same(log, expect):
    assert [(c[0],) + tuple(c[1:2]) for c in log] == [(e[0],) + tuple(e[1:2]) for e in expect], log
    for c, e in zip(log, expect):
        if len(e) > 2:
            assert set(c[2]) == set(e[2]) and all(c[2][k] == pytest.approx(e[2][k], abs=0, rel=1e-15) if isinstance(e[2][k], float)
                                                  else c[2][k] == e[2][k] for k in e[2]), (c, e)


def test_the_modifier_reads_loo_predict_exact_moment_match(rec):
    res, w = _pass(exact_loo_intervals=True, exact_loo_moment_match=True)
    _same(rec, [("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))])
    assert res.exact_loo_intervals is not None and "khat_before" in res.exact_loo_intervals and not w
    del rec[:]
    _pass(exact_loo_intervals=True, exact_loo_moment_match=True, loo_r_eff="auto")
    _same(rec, [("loo_predict_exact_moment_match", [0, 1], dict(r_eff="auto", **INTERVAL))])
    del rec[:]
    res, _ = _pass(exact_loo_intervals=True, exact_loo_moment_match=True, devices=[0, 0])      # over the pooled chains
    _same(rec, [("fit_from_draws",), ("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))])
    assert res.exact_loo_intervals is not None
    del rec[:]
    # each modifier affects its own check only
    _pass(check_loo=True, exact_loo_intervals=True, exact_loo_moment_match=True)
    _same(rec, [("loo", [0, 1], dict(r_eff=None, mcse=False)), ("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))])
    del rec[:]
    _pass(check_loo=True, loo_moment_match=True, exact_loo_intervals=True)
    _same(rec, [("loo_moment_match", [0, 1], dict(r_eff=None)), ("loo_predict_exact", [0, 1], dict(r_eff=None, **INTERVAL))])


def test_a_call_without_the_modifier_is_unchanged(rec):
    res, _ = _pass(exact_loo_intervals=True)
    _same(rec, [("loo_predict_exact", [0, 1], dict(r_eff=None, **INTERVAL))])
    assert "khat_before" not in res.exact_loo_intervals
    del rec[:]
    _pass(exact_loo_intervals=True, exact_loo_moment_match=False, loo_r_eff="auto")
    _same(rec, [("loo_predict_exact", [0, 1], dict(r_eff="auto", **INTERVAL))])
    del rec[:]
    res, _ = _pass()
    assert rec == [] and res.exact_loo_intervals is None


def test_refusals_and_signatures(rec):
    import pandas as pd
    from ppcseq_amd.inference import CHECK_OPTIONS, MODIFIERS, do_inference
    from ppcseq_amd.methods import identify_outliers
    assert "exact_loo_moment_match" in CHECK_OPTIONS and "exact_loo_moment_match" in [m[0] for m in MODIFIERS]
    for fn in (do_inference, identify_outliers):
        assert inspect.signature(fn).parameters["exact_loo_moment_match"].default is False
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals: it matches the moments of the cells "
                                         "whose k-hat their PSIS finds too high"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_moment_match=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_moment_match=True, check_loo=True, loo_moment_match=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_intervals needs a NUTS pass"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, exact_loo_intervals=True,
                     exact_loo_moment_match=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, exact_approximation_loo_intervals=True,
                     exact_loo_moment_match=True, **PASS)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    kw = dict(transcript="symbol", abundance="value")
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals"):
        identify_outliers(df, approximate_posterior_inference=False, exact_loo_moment_match=True, **kw)
    with pytest.raises(ValueError, match="^exact_loo_intervals needs a NUTS pass"):
        identify_outliers(df, approximate_posterior_inference=True, exact_loo_intervals=True, exact_loo_moment_match=True, **kw)
    with pytest.raises(ValueError, match="^exact_loo_intervals is not available for passes over several ranks"):
        identify_outliers(df, approximate_posterior_inference=False, exact_loo_intervals=True, exact_loo_moment_match=True,
                          _pass=lambda *a, **k: None, **kw)
    assert rec == []


def test_identify_outliers_reads_both_passes(rec):
    """both passes read Fit.loo_predict_exact_moment_match; the results go to attrs["exact_loo_intervals_discovery"] and
    ["exact_loo_intervals_test"], the frame is that of the call without the modifier"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, approximate_posterior_inference=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(data, exact_loo_intervals=True, **kw)
        assert [c[0] for c in rec] == ["loo_predict_exact"] * 2
        plain_kw = [c[2] for c in rec]
        del rec[:]
        out = identify_outliers(data, exact_loo_intervals=True, exact_loo_moment_match=True, **kw)
    assert [(c[0], c[1]) for c in rec] == [("loo_predict_exact_moment_match", [0, 1])] * 2
    assert [c[2] for c in rec] == plain_kw                         # the same keywords as the read it replaces
    assert set(out.attrs) == set(plain.attrs) and {"exact_loo_intervals_discovery", "exact_loo_intervals_test"} <= set(out.attrs)
    assert "khat_before" in out.attrs["exact_loo_intervals_test"] and "khat_before" not in plain.attrs["exact_loo_intervals_test"]
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
