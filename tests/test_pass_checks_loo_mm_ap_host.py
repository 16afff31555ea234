"""The two modifiers that moment matching under the weights of an ADVI fit adds to inference.MODIFIERS, on the host: behind the
recording stand-in for _lib.Model / Fit (tests/pass_standin.py), approximation_loo_moment_match turns check_approximation_loo's
read of the fit into Fit.loo_moment_match_approximate_posterior and exact_approximation_loo_moment_match turns
exact_approximation_loo_intervals' read into Fit.loo_predict_exact_moment_match_approximate_posterior, each with exactly the
keywords that read carries today, in both passes of identify_outliers; the k-hat warning reads the final khat; a call without
the flags is unchanged; each flag is refused without the option it needs and with a NUTS pass."""
import inspect
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass

INTERVAL = dict(p_lo=0.05, p_hi=1 - 0.05, truncation_compensation=0.7)      # the pass's adj_prob_theshold and compensation
PLAIN, MM = "loo_approximate_posterior", "loo_moment_match_approximate_posterior"
XPLAIN, XMM = "loo_predict_exact_approximate_posterior", "loo_predict_exact_moment_match_approximate_posterior"
ADVI = dict(approximate_posterior_inference=True)


def _reads(khat=0.3, khat_plain=0.9):
    plain = standin.cells(khat=khat_plain)
    mm = standin.cells(khat=khat, khat_before=khat_plain, iterations=1)
    return {PLAIN: plain, MM: mm, XPLAIN: plain, XMM: mm}


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of check_approximation_loo and exact_approximation_loo_intervals"""
    return standin.install(monkeypatch, _reads())


def _calls(log):
    return [(c[0], list(c[1]), c[2]) for c in log]


def test_the_flags_read_the_matching_methods(rec):
    res, w = _pass(check_approximation_loo=True, approximation_loo_moment_match=True, **ADVI)
    assert _calls(rec) == [(MM, [0, 1], {})]
    assert "khat_before" in res.approximation_loo and res.exact_approximation_loo_intervals is None
    assert not [x for x in w if "Pareto k" in str(x.message)]          # the warning reads the final khat, 0.3
    del rec[:]
    res, w = _pass(exact_approximation_loo_intervals=True, exact_approximation_loo_moment_match=True, **ADVI)
    assert _calls(rec) == [(XMM, [0, 1], INTERVAL)]
    assert "khat_before" in res.exact_approximation_loo_intervals and res.approximation_loo is None
    del rec[:]
    # each flag touches its own read alone
    _pass(check_approximation_loo=True, exact_approximation_loo_intervals=True, approximation_loo_moment_match=True, **ADVI)
    assert _calls(rec) == [(MM, [0, 1], {}), (XPLAIN, [0, 1], INTERVAL)]
    del rec[:]
    _pass(check_approximation_loo=True, exact_approximation_loo_intervals=True, exact_approximation_loo_moment_match=True, **ADVI)
    assert _calls(rec) == [(PLAIN, [0, 1], {}), (XMM, [0, 1], INTERVAL)]


def test_the_warning_reads_the_final_khat(rec, monkeypatch):
    res, w = _pass(check_approximation_loo=True, **ADVI)
    plain_msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    assert plain_msgs                                                  # khat 0.9 is above loo_threshold(300)
    res, w = _pass(check_approximation_loo=True, approximation_loo_moment_match=True, **ADVI)
    assert not [x for x in w if issubclass(x.category, RuntimeWarning)]
    standin.install(monkeypatch, _reads(khat=0.95))
    res, w = _pass(check_approximation_loo=True, approximation_loo_moment_match=True, **ADVI)
    assert [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)] == plain_msgs


def test_a_call_without_the_flags_is_unchanged(rec):
    _pass(check_approximation_loo=True, exact_approximation_loo_intervals=True, **ADVI)
    assert _calls(rec) == [(PLAIN, [0, 1], {}), (XPLAIN, [0, 1], INTERVAL)]
    del rec[:]
    _pass(check_approximation_loo=True, approximation_loo_moment_match=False, exact_approximation_loo_moment_match=False, **ADVI)
    assert _calls(rec) == [(PLAIN, [0, 1], {})]
    del rec[:]
    res, _ = _pass(**ADVI)
    assert rec == [] and res.approximation_loo is None and res.exact_approximation_loo_intervals is None


def test_refusals_and_signatures(rec):
    import pandas as pd
    from ppcseq_amd import _lib
    from ppcseq_amd.inference import CHECK_OPTIONS, MODIFIERS, CheckContext, do_inference
    from ppcseq_amd.methods import identify_outliers
    assert CHECK_OPTIONS[-2:] == ("approximation_loo_moment_match", "exact_approximation_loo_moment_match")   # appended
    needs = dict((m[0], m[1]) for m in MODIFIERS)
    assert needs["approximation_loo_moment_match"] == ("check_approximation_loo",)
    assert needs["exact_approximation_loo_moment_match"] == ("exact_approximation_loo_intervals",)
    ctx = CheckContext(K, 0.05, 1, 1.0)
    assert ctx.approximation_loo_moment_match is False and ctx.exact_approximation_loo_moment_match is False
    for fn in (do_inference, identify_outliers):
        for flag in ("approximation_loo_moment_match", "exact_approximation_loo_moment_match"):
            assert inspect.signature(fn).parameters[flag].default is False
    sig = inspect.signature(_lib.Fit.loo_moment_match_approximate_posterior).parameters
    assert list(sig) == ["self", "genes", "k_threshold", "max_iters"] and sig["max_iters"].default == 30 and sig["k_threshold"].default is None
    sig = inspect.signature(_lib.Fit.loo_predict_exact_moment_match_approximate_posterior).parameters
    assert list(sig) == ["self", "genes", "k_threshold", "max_iters", "p_lo", "p_hi", "truncation_compensation"]
    assert (sig["max_iters"].default, sig["p_lo"].default, sig["p_hi"].default, sig["truncation_compensation"].default) == (30, 0.025, 0.975, 1.0)
    run = lambda **kw: do_inference(COUNTS, X, np.zeros(S), K, **kw, **PASS)
    with pytest.raises(ValueError, match="^approximation_loo_moment_match needs check_approximation_loo"):
        run(approximation_loo_moment_match=True, **ADVI)
    with pytest.raises(ValueError, match="^approximation_loo_moment_match needs check_approximation_loo"):
        run(exact_approximation_loo_intervals=True, approximation_loo_moment_match=True, **ADVI)
    with pytest.raises(ValueError, match="^exact_approximation_loo_moment_match needs exact_approximation_loo_intervals"):
        run(exact_approximation_loo_moment_match=True, **ADVI)
    with pytest.raises(ValueError, match="^exact_approximation_loo_moment_match needs exact_approximation_loo_intervals"):
        run(check_approximation_loo=True, approximation_loo_moment_match=True, exact_approximation_loo_moment_match=True, **ADVI)
    # a NUTS pass: the option each flag needs is refused first
    with pytest.raises(ValueError, match="^check_approximation_loo needs an ADVI pass"):
        run(check_approximation_loo=True, approximation_loo_moment_match=True)
    with pytest.raises(ValueError, match="^exact_approximation_loo_intervals needs an ADVI pass"):
        run(exact_approximation_loo_intervals=True, exact_approximation_loo_moment_match=True)
    with pytest.raises(ValueError, match="^approximation_loo_moment_match needs check_approximation_loo"):
        run(check_loo=True, loo_moment_match=True, approximation_loo_moment_match=True)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="^approximation_loo_moment_match needs check_approximation_loo"):
        identify_outliers(df, approximation_loo_moment_match=True, transcript="symbol", abundance="value")
    with pytest.raises(ValueError, match="^check_approximation_loo needs an ADVI pass"):
        identify_outliers(df, approximate_posterior_inference=False, check_approximation_loo=True, approximation_loo_moment_match=True,
                          transcript="symbol", abundance="value", _pass=lambda *a, **kw: None)
    assert rec == []


def test_identify_outliers_reads_both_passes(rec):
    """both passes read the matching methods with the keywords of the call without the flags; the frame is that call's"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, check_approximation_loo=True, exact_approximation_loo_intervals=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(data, **kw)
        assert [c[0] for c in rec] == [PLAIN, XPLAIN] * 2
        plain_kw = [c[2] for c in rec]
        del rec[:]
        out = identify_outliers(data, approximation_loo_moment_match=True, exact_approximation_loo_moment_match=True, **kw)
    assert [(c[0], list(c[1])) for c in rec] == [(MM, [0, 1]), (XMM, [0, 1])] * 2
    assert [c[2] for c in rec] == plain_kw
    assert set(out.attrs) == set(plain.attrs)
    for key in ("approximation_loo_discovery", "approximation_loo_test", "exact_approximation_loo_intervals_discovery",
                "exact_approximation_loo_intervals_test"):
        assert "khat_before" in out.attrs[key] and "khat_before" not in plain.attrs[key], key
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
