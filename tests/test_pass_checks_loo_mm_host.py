"""The modifier that gene-local moment matching adds to inference.MODIFIERS, on the host, beside
tests/test_pass_checks_host.py: behind a recording stand-in for _lib.Model / Fit, loo_moment_match turns check_loo's one read
of the fit into Fit.loo_moment_match with the pass's r_eff (pooled chains allowed), the k-hat warning reads the final khat, a
call without the modifier carries exactly the keywords it carried before, and the modifier is refused without check_loo and
together with loo_mcse."""
import warnings

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, PASS, S, X, run_pass as _pass


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log the reads of check_loo"""
    return standin.install(monkeypatch, dict(loo=standin.cells(khat=0.9), loo_moment_match=standin.cells(khat=0.3, khat_before=0.9)))


def test_the_modifier_reads_loo_moment_match(rec):
    res, w = _pass(check_loo=True, loo_moment_match=True)
    assert rec == [("loo_moment_match", [0, 1], dict(r_eff=None))]
    assert res.loo is not None and "khat_before" in res.loo
    assert not w                                                   # the final khat (0.3) is read, not khat_before (0.9)
    del rec[:]
    _pass(check_loo=True, loo_moment_match=True, loo_r_eff="auto")
    assert rec == [("loo_moment_match", [0, 1], dict(r_eff="auto"))]
    del rec[:]
    res, _ = _pass(check_loo=True, loo_moment_match=True, devices=[0, 0])   # over the pooled chains: no lp__ is needed
    assert rec == [("fit_from_draws",), ("loo_moment_match", [0, 1], dict(r_eff=None))]
    assert res.loo is not None


def test_a_call_without_the_modifier_is_unchanged(rec):
    res, w = _pass(check_loo=True)
    assert rec == [("loo", [0, 1], dict(r_eff=None, mcse=False))]
    assert any("k" in str(x.message) for x in w)                   # plain PSIS's khat of 0.9 is reported as before
    del rec[:]
    _pass(check_loo=True, loo_r_eff="auto", loo_mcse=True)
    assert rec == [("loo", [0, 1], dict(r_eff="auto", mcse=True))]
    del rec[:]
    _pass(check_loo=True, loo_moment_match=False)
    assert rec == [("loo", [0, 1], dict(r_eff=None, mcse=False))]
    del rec[:]
    res, _ = _pass()
    assert rec == [] and res.loo is None


def test_refusals(rec):
    import pandas as pd
    from ppcseq_amd.inference import CHECK_OPTIONS, do_inference
    from ppcseq_amd.methods import identify_outliers
    assert "loo_moment_match" in CHECK_OPTIONS
    with pytest.raises(ValueError, match="^loo_moment_match needs check_loo: it matches the moments of the cells whose k-hat"):
        do_inference(COUNTS, X, np.zeros(S), K, loo_moment_match=True, **PASS)
    with pytest.raises(ValueError, match="^loo_moment_match needs check_loo"):
        do_inference(COUNTS, X, np.zeros(S), K, loo_moment_match=True, check_loo_intervals=True, **PASS)
    with pytest.raises(ValueError, match="^loo_mcse cannot be combined with loo_moment_match: the Monte-Carlo standard error and "
                                         "n_eff are those of plain PSIS weights and are not given for a matched cell"):
        do_inference(COUNTS, X, np.zeros(S), K, check_loo=True, loo_mcse=True, loo_moment_match=True, **PASS)
    with pytest.raises(ValueError, match="^check_loo needs a NUTS pass"):
        do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=True, check_loo=True, loo_moment_match=True, **PASS)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    kw = dict(transcript="symbol", abundance="value")
    with pytest.raises(ValueError, match="^loo_moment_match needs check_loo"):
        identify_outliers(df, approximate_posterior_inference=False, loo_moment_match=True, **kw)
    with pytest.raises(ValueError, match="^loo_mcse cannot be combined with loo_moment_match"):
        identify_outliers(df, approximate_posterior_inference=False, check_loo=True, loo_mcse=True, loo_moment_match=True, **kw)
    assert rec == []


def test_identify_outliers_reads_both_passes(rec):
    """both passes read Fit.loo_moment_match; the results go to attrs["loo_discovery"] and ["loo_test"], the frame is that of the
    call without the modifier"""
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    data = pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, approximate_posterior_inference=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = identify_outliers(data, check_loo=True, **kw)
        assert [c[0] for c in rec] == ["loo", "loo"]
        del rec[:]
        out = identify_outliers(data, check_loo=True, loo_moment_match=True, loo_r_eff="auto", **kw)
    assert [(c[0], c[1], c[2]) for c in rec] == [("loo_moment_match", [0, 1], dict(r_eff="auto"))] * 2
    assert set(out.attrs) == set(plain.attrs) and {"loo_discovery", "loo_test"} <= set(out.attrs)
    assert "khat_before" in out.attrs["loo_test"] and "khat_before" not in plain.attrs["loo_test"]
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
