"""The modifier that the covariance step of the exact predictive adds to inference.MODIFIERS, on the host, beside
tests/test_pass_checks_loo_mm_cov_host.py: behind the recording stand-in for _lib.Model / Fit (tests/pass_standin.py),
exact_loo_moment_match_cov turns exact_loo_moment_match's read of the fit into Fit.loo_predict_exact_moment_match_cov with exactly
the keywords that read carries today -- r_eff and the pass's interval, plus split=True with exact_loo_moment_match_split; no `cov`
keyword -- in both passes of identify_outliers and over pooled chains; a call without the flag is unchanged; the flag is refused
without exact_loo_moment_match and on an ADVI pass; loo_moment_match_cov keeps affecting check_loo's read only."""
import inspect
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass

INTERVAL = dict(p_lo=0.05, p_hi=1 - 0.05, truncation_compensation=0.7)      # the pass's adj_prob_theshold and compensation
COV = "loo_predict_exact_moment_match_cov"


def _reads(khat=0.3):
    good = standin.cells(khat=khat)
    mm = lambda fit, genes, kw: standin.cells(khat=khat, khat_before=0.9, **(dict(cov_iterations=1) if kw.get("cov") else {}),
                                              **(dict(khat_split=0.2) if kw.get("split") else {}))(fit, genes, kw)
    xcov = lambda fit, genes, kw: standin.cells(khat=khat, khat_before=0.9, cov_iterations=1,
                                                **(dict(khat_split=0.2) if kw.get("split") else {}))(fit, genes, kw)
    return {"loo": good, "loo_moment_match": mm, "loo_predict_exact": good, "loo_predict_exact_moment_match": mm, COV: xcov}


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of check_loo and exact_loo_intervals"""
    return standin.install(monkeypatch, _reads())


def _calls(log):
    return [(c[0],) + ((list(c[1]), c[2]) if len(c) > 1 else ()) for c in log]


def test_the_flag_reads_the_covariance_method(rec):
    res, w = _pass(exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_cov=True)
    assert _calls(rec) == [(COV, [0, 1], dict(r_eff=None, **INTERVAL))]
    assert "cov" not in rec[0][2] and "cov_iterations" in res.exact_loo_intervals and "khat_split" not in res.exact_loo_intervals and not w
    del rec[:]
    res, w = _pass(exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_split=True, exact_loo_moment_match_cov=True,
                   loo_r_eff="auto")
    assert _calls(rec) == [(COV, [0, 1], dict(r_eff="auto", split=True, **INTERVAL))]
    assert rec[0][2]["split"] is True and "khat_split" in res.exact_loo_intervals and not w
    del rec[:]
    # over the pooled chains; check_loo's read is untouched by the flag, and loo_moment_match_cov touches check_loo's alone
    _pass(check_loo=True, loo_moment_match=True, exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_cov=True,
          devices=[0, 0])
    got = _calls(rec)
    assert got[0] == ("fit_from_draws",) and got[1] == ("loo_moment_match", [0, 1], dict(r_eff=None))
    assert got[2] == (COV, [0, 1], dict(r_eff=None, **INTERVAL)) and len(got) == 3
    del rec[:]
    _pass(check_loo=True, loo_moment_match=True, loo_moment_match_cov=True, exact_loo_intervals=True, exact_loo_moment_match=True)
    got = _calls(rec)
    assert got[0] == ("loo_moment_match", [0, 1], dict(r_eff=None, cov=True))
    assert got[1] == ("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))


def test_a_call_without_the_flag_is_unchanged(rec):
    _pass(exact_loo_intervals=True, exact_loo_moment_match=True)
    assert _calls(rec) == [("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))]
    del rec[:]
    _pass(exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_cov=False, exact_loo_moment_match_split=True)
    assert _calls(rec) == [("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, split=True, **INTERVAL))]
    del rec[:]
    _pass(exact_loo_intervals=True)
    assert _calls(rec) == [("loo_predict_exact", [0, 1], dict(r_eff=None, **INTERVAL))]
    del rec[:]
    res, _ = _pass()
    assert rec == [] and res.exact_loo_intervals is None


def test_refusals_and_signatures(rec):
    import pandas as pd
    from ppcseq_amd import _lib
    from ppcseq_amd.inference import CHECK_OPTIONS, MODIFIERS, CheckContext, do_inference
    from ppcseq_amd.methods import identify_outliers
    assert "exact_loo_moment_match_cov" in CHECK_OPTIONS
    assert [m for m in MODIFIERS if m[0] == "exact_loo_moment_match_cov"][0][1] == ("exact_loo_moment_match",)
    assert CheckContext(K, 0.05, 1, 1.0).exact_loo_moment_match_cov is False
    for fn in (do_inference, identify_outliers):
        assert inspect.signature(fn).parameters["exact_loo_moment_match_cov"].default is False
    sig = inspect.signature(_lib.Fit.loo_predict_exact_moment_match_cov).parameters
    assert sig["split"].default is False and sig["max_iters"].default == 30 and sig["k_threshold"].default is None and "cov" not in sig
    assert "cov" not in inspect.signature(_lib.Fit.loo_predict_exact_moment_match).parameters
    needs = "^exact_loo_moment_match_cov needs exact_loo_moment_match: it is the covariance step of the matching of its cells"
    with pytest.raises(ValueError, match=needs):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match=needs):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_intervals=True, exact_loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match=needs):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_moment_match=True, loo_moment_match_cov=True,
                     exact_loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_moment_match=True, exact_loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_intervals needs a NUTS pass"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, exact_loo_intervals=True,
                     exact_loo_moment_match=True, exact_loo_moment_match_cov=True, **PASS)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match=needs):
        identify_outliers(df, approximate_posterior_inference=False, exact_loo_intervals=True, exact_loo_moment_match_cov=True,
                          transcript="symbol", abundance="value")
    with pytest.raises(ValueError, match="^exact_loo_intervals is not available for passes over several ranks"):
        identify_outliers(df, approximate_posterior_inference=False, exact_loo_intervals=True, exact_loo_moment_match=True,
                          exact_loo_moment_match_cov=True, transcript="symbol", abundance="value", _pass=lambda *a, **kw: None)
    assert rec == []


def test_identify_outliers_reads_both_passes(rec):
    """both passes read Fit.loo_predict_exact_moment_match_cov with the keywords of the call without the flag; the frame is that
    call's"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, approximate_posterior_inference=False, exact_loo_intervals=True,
              exact_loo_moment_match=True, exact_loo_moment_match_split=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(data, **kw)
        assert [c[0] for c in rec] == ["loo_predict_exact_moment_match"] * 2
        plain_kw = [c[2] for c in rec]
        del rec[:]
        out = identify_outliers(data, exact_loo_moment_match_cov=True, **kw)
    assert [(c[0], list(c[1])) for c in rec] == [(COV, [0, 1])] * 2
    assert [c[2] for c in rec] == plain_kw and all("cov" not in k and k["split"] is True for k in plain_kw)
    assert set(out.attrs) == set(plain.attrs)
    for key in ("exact_loo_intervals_discovery", "exact_loo_intervals_test"):
        assert "cov_iterations" in out.attrs[key] and "cov_iterations" not in plain.attrs[key], key
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
