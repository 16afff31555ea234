"""The modifier that the covariance step adds to inference.MODIFIERS, on the host, beside
tests/test_pass_checks_loo_mm_split_host.py: behind the recording stand-in for _lib.Model / Fit (tests/pass_standin.py),
loo_moment_match_cov turns loo_moment_match's read of the fit into Fit.loo_moment_match(..., cov=True), alone or together with
split=True, in both passes of identify_outliers; a call without the flag carries exactly the keywords it carried before (no
`cov` among them); the flag is refused without loo_moment_match and, like it, together with loo_mcse; the exact predictive's
read takes no such keyword."""
import inspect
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass

INTERVAL = dict(p_lo=0.05, p_hi=1 - 0.05, truncation_compensation=0.7)      # the pass's adj_prob_theshold and compensation


def _reads(khat=0.3):
    good = standin.cells(khat=khat)
    mm = lambda fit, genes, kw: standin.cells(khat=khat, khat_before=0.9, **(dict(cov_iterations=1) if kw.get("cov") else {}),
                                              **(dict(khat_split=0.2) if kw.get("split") else {}))(fit, genes, kw)
    return dict(loo=good, loo_moment_match=mm, loo_predict_exact=good, loo_predict_exact_moment_match=mm)


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of check_loo and exact_loo_intervals"""
    return standin.install(monkeypatch, _reads())


def _calls(log):
    return [(c[0],) + ((list(c[1]), c[2]) if len(c) > 1 else ()) for c in log]


def test_the_flag_reads_with_cov_true(rec):
    res, w = _pass(check_loo=True, loo_moment_match=True, loo_moment_match_cov=True)
    assert _calls(rec) == [("loo_moment_match", [0, 1], dict(r_eff=None, cov=True))]
    assert rec[0][2]["cov"] is True and "cov_iterations" in res.loo and "khat_split" not in res.loo and not w
    del rec[:]
    res, w = _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=True, loo_moment_match_cov=True, loo_r_eff="auto")
    assert _calls(rec) == [("loo_moment_match", [0, 1], dict(r_eff="auto", split=True, cov=True))]
    assert "cov_iterations" in res.loo and "khat_split" in res.loo and not w
    del rec[:]
    # over the pooled chains; the exact predictive's read is untouched by the flag
    _pass(check_loo=True, loo_moment_match=True, loo_moment_match_cov=True, exact_loo_intervals=True, exact_loo_moment_match=True,
          exact_loo_moment_match_split=True, devices=[0, 0])
    got = _calls(rec)
    assert got[0] == ("fit_from_draws",) and got[1] == ("loo_moment_match", [0, 1], dict(r_eff=None, cov=True))
    assert got[2][0] == "loo_predict_exact_moment_match" and set(got[2][2]) == {"r_eff", "split"} | set(INTERVAL)


def test_a_call_without_the_flag_is_unchanged(rec):
    _pass(check_loo=True, loo_moment_match=True)
    assert _calls(rec) == [("loo_moment_match", [0, 1], dict(r_eff=None))]
    del rec[:]
    _pass(check_loo=True, loo_moment_match=True, loo_moment_match_cov=False, loo_moment_match_split=True)
    assert _calls(rec) == [("loo_moment_match", [0, 1], dict(r_eff=None, split=True))]
    del rec[:]
    _pass(check_loo=True, exact_loo_intervals=True, exact_loo_moment_match=True)
    got = _calls(rec)
    assert got[0] == ("loo", [0, 1], dict(r_eff=None, mcse=False))
    assert got[1][0] == "loo_predict_exact_moment_match" and set(got[1][2]) == {"r_eff"} | set(INTERVAL)
    del rec[:]
    res, _ = _pass()
    assert rec == [] and res.loo is None


def test_refusals_and_signatures(rec):
    import pandas as pd
    from ppcseq_amd import _lib
    from ppcseq_amd.inference import CHECK_OPTIONS, MODIFIERS, do_inference
    from ppcseq_amd.methods import identify_outliers
    assert "loo_moment_match_cov" in CHECK_OPTIONS
    assert [m for m in MODIFIERS if m[0] == "loo_moment_match_cov"][0][1] == ("loo_moment_match",)
    for fn in (do_inference, identify_outliers):
        assert inspect.signature(fn).parameters["loo_moment_match_cov"].default is False
    assert inspect.signature(_lib.Fit.loo_moment_match).parameters["cov"].default is False
    assert "cov" not in inspect.signature(_lib.Fit.loo_predict_exact_moment_match).parameters
    needs = "^loo_moment_match_cov needs loo_moment_match: it is the covariance step of the matching of its cells"
    with pytest.raises(ValueError, match=needs):
        do_inference(COUNTS, X, np.zeros(S), K, loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match=needs):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match=needs):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_intervals=True, exact_loo_moment_match=True, loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match="^loo_moment_match needs check_loo"):
        do_inference(COUNTS, X, np.zeros(S), K, loo_moment_match=True, loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match="^loo_mcse cannot be combined with loo_moment_match"):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_mcse=True, loo_moment_match=True, loo_moment_match_cov=True, **PASS)
    with pytest.raises(ValueError, match="^check_loo needs a NUTS pass"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, check_loo=True, loo_moment_match=True,
                     loo_moment_match_cov=True, **PASS)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match=needs):
        identify_outliers(df, approximate_posterior_inference=False, check_loo=True, loo_moment_match_cov=True, transcript="symbol",
                          abundance="value")
    assert rec == []


def test_identify_outliers_reads_both_passes(rec):
    """both passes read Fit.loo_moment_match with cov=True; the frame is that of the call without the flag"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, approximate_posterior_inference=False, check_loo=True,
              loo_moment_match=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(data, **kw)
        assert [c[0] for c in rec] == ["loo_moment_match"] * 2 and all("cov" not in c[2] for c in rec)
        plain_kw = [c[2] for c in rec]
        del rec[:]
        out = identify_outliers(data, loo_moment_match_cov=True, **kw)
    assert [(c[0], list(c[1])) for c in rec] == [("loo_moment_match", [0, 1])] * 2
    assert [c[2] for c in rec] == [dict(k, cov=True) for k in plain_kw]
    assert set(out.attrs) == set(plain.attrs)
    for key in ("loo_discovery", "loo_test"):
        assert "cov_iterations" in out.attrs[key] and "cov_iterations" not in plain.attrs[key], key
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
