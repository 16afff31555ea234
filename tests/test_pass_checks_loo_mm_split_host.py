"""The two modifiers that the split transformation adds to inference.MODIFIERS, on the host, beside
tests/test_pass_checks_loo_mm_host.py and tests/test_pass_checks_loo_mm_exact_host.py: behind the recording stand-in for
_lib.Model / Fit (tests/pass_standin.py), loo_moment_match_split turns loo_moment_match's read of the fit into
Fit.loo_moment_match(..., split=True) and exact_loo_moment_match_split turns exact_loo_moment_match's into
Fit.loo_predict_exact_moment_match(..., split=True), in both passes of identify_outliers; a call without the flags carries
exactly the keywords it carried before (no `split` among them); each flag is refused without the modifier it belongs to; and the
k-hat warning keeps reading `khat`."""
import inspect
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass

INTERVAL = dict(p_lo=0.05, p_hi=1 - 0.05, truncation_compensation=0.7)      # the pass's adj_prob_theshold and compensation


def _reads(khat=0.3, khat_split=0.95):
    good = standin.cells(khat=khat)
    mm = lambda fit, genes, kw: standin.cells(khat=khat, khat_before=0.9, **(dict(khat_split=khat_split) if kw.get("split") else {}))(
        fit, genes, kw)
    return dict(loo=good, loo_moment_match=mm, loo_predict_exact=good, loo_predict_exact_moment_match=mm)


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of check_loo and exact_loo_intervals"""
    return standin.install(monkeypatch, _reads())


def _same(log, expect):
    assert [(c[0],) + tuple(c[1:2]) for c in log] == [(e[0],) + tuple(e[1:2]) for e in expect], log
    for c, e in zip(log, expect):
        if len(e) > 2:
            assert set(c[2]) == set(e[2]) and all(c[2][k] == pytest.approx(e[2][k], abs=0, rel=1e-15) if isinstance(e[2][k], float)
                                                  else c[2][k] == e[2][k] for k in e[2]), (c, e)


def test_the_flags_read_with_split_true(rec):
    res, w = _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=True)
    _same(rec, [("loo_moment_match", [0, 1], dict(r_eff=None, split=True))])
    assert rec[0][2]["split"] is True and "khat_split" in res.loo and not w
    del rec[:]
    res, w = _pass(exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_split=True, loo_r_eff="auto")
    _same(rec, [("loo_predict_exact_moment_match", [0, 1], dict(r_eff="auto", split=True, **INTERVAL))])
    assert rec[0][2]["split"] is True and "khat_split" in res.exact_loo_intervals and not w
    del rec[:]
    res, _ = _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=True, exact_loo_intervals=True,
                   exact_loo_moment_match=True, exact_loo_moment_match_split=True, devices=[0, 0])      # over the pooled chains
    _same(rec, [("fit_from_draws",), ("loo_moment_match", [0, 1], dict(r_eff=None, split=True)),
                ("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, split=True, **INTERVAL))])
    del rec[:]
    # each flag affects its own read only
    _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=True, exact_loo_intervals=True, exact_loo_moment_match=True)
    _same(rec, [("loo_moment_match", [0, 1], dict(r_eff=None, split=True)),
                ("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))])
    del rec[:]
    _pass(check_loo=True, loo_moment_match=True, exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_split=True)
    _same(rec, [("loo_moment_match", [0, 1], dict(r_eff=None)),
                ("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, split=True, **INTERVAL))])


def test_a_call_without_the_flags_is_unchanged(rec):
    """exactly today's keywords: _same compares the sets of keywords, so a `split` among them fails"""
    _pass(check_loo=True, loo_moment_match=True)
    _same(rec, [("loo_moment_match", [0, 1], dict(r_eff=None))])
    assert "split" not in rec[0][2]
    del rec[:]
    _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=False, loo_r_eff="auto")
    _same(rec, [("loo_moment_match", [0, 1], dict(r_eff="auto"))])
    del rec[:]
    res, _ = _pass(exact_loo_intervals=True, exact_loo_moment_match=True, exact_loo_moment_match_split=False)
    _same(rec, [("loo_predict_exact_moment_match", [0, 1], dict(r_eff=None, **INTERVAL))])
    assert "split" not in rec[0][2] and "khat_split" not in res.exact_loo_intervals
    del rec[:]
    _pass(check_loo=True, exact_loo_intervals=True)
    _same(rec, [("loo", [0, 1], dict(r_eff=None, mcse=False)), ("loo_predict_exact", [0, 1], dict(r_eff=None, **INTERVAL))])
    del rec[:]
    res, _ = _pass()
    assert rec == [] and res.loo is None and res.exact_loo_intervals is None


def test_the_khat_warning_keeps_reading_khat(monkeypatch):
    """a high khat_split raises nothing (rec's reads: khat 0.3, khat_split 0.95); a high khat does, whatever khat_split is"""
    log = standin.install(monkeypatch, _reads(khat=0.3, khat_split=0.95))
    _, w = _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=True)
    assert len(log) == 1 and not w
    log = standin.install(monkeypatch, _reads(khat=0.95, khat_split=0.1))
    _, w = _pass(check_loo=True, loo_moment_match=True, loo_moment_match_split=True)
    assert len(log) == 1 and len(w) >= 1 and all(issubclass(x.category, RuntimeWarning) for x in w)
    _, w0 = _pass(check_loo=True, loo_moment_match=True)
    assert [str(x.message) for x in w0] == [str(x.message) for x in w]


def test_refusals_and_signatures(rec):
    import pandas as pd
    from ppcseq_amd.inference import CHECK_OPTIONS, MODIFIERS, do_inference
    from ppcseq_amd.methods import identify_outliers
    for flag in ("loo_moment_match_split", "exact_loo_moment_match_split"):
        assert flag in CHECK_OPTIONS and flag in [m[0] for m in MODIFIERS]
        for fn in (do_inference, identify_outliers):
            assert inspect.signature(fn).parameters[flag].default is False
    with pytest.raises(ValueError, match="^loo_moment_match_split needs loo_moment_match: it is the split transformation of the cells "
                                         "that it has matched"):
        do_inference(COUNTS, X, np.zeros(S), K, loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^loo_moment_match_split needs loo_moment_match"):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^loo_moment_match_split needs loo_moment_match"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_intervals=True, exact_loo_moment_match=True, loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^loo_moment_match needs check_loo"):
        do_inference(COUNTS, X, np.zeros(S), K, loo_moment_match=True, loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match_split needs exact_loo_moment_match: it is the split transformation of "
                                         "the cells that it has matched"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match_split needs exact_loo_moment_match"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_intervals=True, exact_loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match_split needs exact_loo_moment_match"):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_moment_match=True, exact_loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^exact_loo_moment_match needs exact_loo_intervals"):
        do_inference(COUNTS, X, np.zeros(S), K, exact_loo_moment_match=True, exact_loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^check_loo needs a NUTS pass"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, check_loo=True, loo_moment_match=True,
                     loo_moment_match_split=True, **PASS)
    with pytest.raises(ValueError, match="^loo_mcse cannot be combined with loo_moment_match"):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_mcse=True, loo_moment_match=True, loo_moment_match_split=True, **PASS)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    kw = dict(transcript="symbol", abundance="value")
    with pytest.raises(ValueError, match="^loo_moment_match_split needs loo_moment_match"):
        identify_outliers(df, approximate_posterior_inference=False, check_loo=True, loo_moment_match_split=True, **kw)
    with pytest.raises(ValueError, match="^exact_loo_moment_match_split needs exact_loo_moment_match"):
        identify_outliers(df, approximate_posterior_inference=False, exact_loo_intervals=True, exact_loo_moment_match_split=True, **kw)
    assert rec == []


def test_identify_outliers_reads_both_passes(rec):
    """both passes read the two methods with split=True; the results stay in attrs["loo_*"] and ["exact_loo_intervals_*"], the
    frame is that of the call without the flags"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, approximate_posterior_inference=False, check_loo=True,
              loo_moment_match=True, exact_loo_intervals=True, exact_loo_moment_match=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(data, **kw)
        names = ["loo_moment_match", "loo_predict_exact_moment_match"] * 2
        assert [c[0] for c in rec] == names and all("split" not in c[2] for c in rec)
        plain_kw = [c[2] for c in rec]
        del rec[:]
        out = identify_outliers(data, loo_moment_match_split=True, exact_loo_moment_match_split=True, **kw)
    assert [(c[0], c[1]) for c in rec] == [(name, [0, 1]) for name in names]
    assert [c[2] for c in rec] == [dict(k, split=True) for k in plain_kw]      # the same keywords, and split=True
    assert set(out.attrs) == set(plain.attrs) and {"loo_discovery", "loo_test", "exact_loo_intervals_discovery",
                                                   "exact_loo_intervals_test"} <= set(out.attrs)
    for key in ("loo_discovery", "loo_test", "exact_loo_intervals_discovery", "exact_loo_intervals_test"):
        assert "khat_split" in out.attrs[key] and "khat_split" not in plain.attrs[key], key
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
