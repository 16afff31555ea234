"""The optional diagnostics of a pass from the frame to the fit, on the host: behind a recording stand-in for _lib.Model / Fit
every combination of the options either is refused before anything touches the model or produces exactly the fit calls, result
fields, attrs keys and warnings of the selected options, each stated literally below -- for a single fit, for pooled chains
(devices=[0, 0]) and for identify_outliers' two passes."""
import itertools
import threading
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pass_standin as standin
from tests.pass_standin import COUNTS, G, K, S, X

ar = np.arange

# option -> (InferenceResult field and attrs prefix, the pass it needs, the one read of the fit, the warnings it adds with the
# stand-in's poor k-hats / R-hats). c: G (genes of the fit's model), K, p, seed, tc, r_eff, mcse, pooled
EXPECT = {
    "check_approximation": ("approximation", "advi", lambda c: ("psis", (3 + c.G + ar(c.K),), dict(overall=True)), 1),
    "check_approximation_loo": ("approximation_loo", "advi", lambda c: ("loo_approximate_posterior", (ar(c.K),), {}), 1),
    "check_approximation_loo_intervals": ("approximation_loo_intervals", "advi", lambda c: (
        "loo_predict_approximate_posterior", (ar(c.K),), dict(p_lo=c.p, p_hi=1 - c.p, seed=c.seed, truncation_compensation=c.tc)), 0),
    "check_convergence": ("convergence", "nuts", lambda c: ("summary", (3 + c.G + ar(c.K),), dict(lp=not c.pooled)), 3),
    "check_loo": ("loo", "nuts", lambda c: ("loo", (ar(c.K),), dict(r_eff=c.r_eff, mcse=c.mcse)), 1),
    "check_loo_intervals": ("loo_intervals", "nuts", lambda c: (
        "loo_predict", (ar(c.K),), dict(r_eff=c.r_eff, p_lo=c.p, p_hi=1 - c.p, seed=c.seed, truncation_compensation=c.tc)), 0),
    "exact_intervals": ("exact_intervals", None, lambda c: (
        "ppc_exact", (ar(c.K),), dict(p_lo=c.p, p_hi=1 - c.p, truncation_compensation=c.tc)), 0),
}
ORDER = list(EXPECT)                                  # the order of the reads
OVER_CELLS = ("check_loo", "check_loo_intervals", "exact_intervals")     # pooled: None at K == 0, the small model carries excl
BOOLS = ORDER + ["loo_mcse"]
ATTRS = ["abundance_column", "diagnostics_discovery", "diagnostics_test", "formula", "sample_column", "seed", "total_draws",
         "transcript_column"]


def broken_rules(o, advi):
    """the options whose rule the combination breaks"""
    bad = [k for k in ORDER if o[k] and EXPECT[k][1] not in (None, "advi" if advi else "nuts")]
    if o["loo_mcse"] and not o["check_loo"]:
        bad.append("loo_mcse")
    if o["loo_r_eff"] is not None and not (o["check_loo"] or o["check_loo_intervals"]):
        bad.append("loo_r_eff")
    return bad


def combinations():
    for bits in itertools.product([False, True], repeat=len(BOOLS)):
        for r_eff in (None, "auto"):
            yield dict(zip(BOOLS, bits), loo_r_eff=r_eff)


def canon(v):
    if isinstance(v, np.ndarray):
        return ("array", v.shape, tuple(v.ravel().tolist()))
    if isinstance(v, (list, tuple)):
        return tuple(canon(x) for x in v)
    if isinstance(v, dict):
        return tuple(sorted((k, canon(x)) for k, x in v.items()))
    return v.item() if isinstance(v, np.generic) else v


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *a, **kw):
        self.calls.append((threading.current_thread().name, name, canon(a), canon(kw)))

    def main(self):
        return [c[1:] for c in self.calls if c[0] == "MainThread"]


@pytest.fixture
def rec(monkeypatch):
    """_lib.Model / Fit replaced by stand-ins that log every call and return arrays of the right shape, with k-hats and R-hats
    poor enough for every warning"""
    poor = standin.cells(khat=0.9)

    def summary(fit, cols, kw):
        n = len(cols) + bool(kw["lp"])
        return dict(rhat=np.full(n, 2.0), ess_bulk=np.full(n, 5.0), ess_tail=np.full(n, 5.0))

    return standin.install(monkeypatch, log=Recorder(), poor_sampler=True, reads=dict(
        summary=summary, psis=lambda fit, cols, kw: dict(khat=np.full(len(cols) + bool(kw["overall"]), 0.9)),
        loo=poor, loo_predict=poor, loo_approximate_posterior=poor, loo_predict_approximate_posterior=poor,
        ppc_exact=standin.cells(lower=0.0)))


def reads(o, advi, **ctx):
    """the reads the selected options must produce, in order, as the stand-in logs them"""
    c = SimpleNamespace(K=K, r_eff=o["loo_r_eff"], mcse=o["loo_mcse"], **ctx)
    out = []
    for k in ORDER:
        if o[k] and not (c.pooled and c.K == 0 and k in OVER_CELLS):
            name, a, kw = EXPECT[k][2](c)
            out.append((name, canon(a), canon(kw)))
    return out


def n_warnings(o, advi, K=K, pooled=False):
    own = sum(EXPECT[k][3] for k in ORDER if o[k]) if K else 0      # without a checked gene there is nothing to warn of
    return own + (0 if advi or pooled else 2)         # a single NUTS fit: divergences and tree depth first


def split(calls, first, last="fit.close"):
    """(the calls up to and including the first `first`, the reads after it, the calls from `last` on)"""
    names = [c[0] for c in calls]
    i, j = names.index(first) + 1, names.index(last)
    return calls[:i], calls[i:j], calls[j:]


PASS = dict(standin.PASS, to_exclude=np.array([1, 5, 20]))


def run_pass(rec, o, n_checked=K, **kw):
    del rec.calls[:]
    res, w = standin.run_pass(n_checked, **PASS, **kw, **o)
    assert all(x.category is RuntimeWarning for x in w)
    return res, w


def test_do_inference_composes_the_selected_options(rec):
    valid = {False: 0, True: 0}
    plain = {}
    for advi in (False, True):
        res, _ = run_pass(rec, {}, approximate_posterior_inference=advi)
        plain[advi] = split(rec.main(), "advi_info" if advi else "diagnostics")
        assert plain[advi][1] == [] and [c[0] for c in plain[advi][2]] == ["fit.close", "model.close"]
    assert plain[False][0][2] == ("fit_nuts", (), canon(dict(chains=3, iter=250, warmup=150, seed=7)))
    for o in combinations():
        for advi in (False, True):
            del rec.calls[:]
            bad = broken_rules(o, advi)
            if bad:
                from ppcseq_amd.inference import do_inference
                with pytest.raises(ValueError) as e:
                    do_inference(COUNTS, X, np.zeros(S), K, approximate_posterior_inference=advi, **PASS, **o)
                assert str(e.value).split()[0] in bad, (o, advi, str(e.value))
                assert rec.calls == []
                continue
            valid[advi] += o["loo_r_eff"] is None
            res, w = run_pass(rec, o, approximate_posterior_inference=advi)
            before, read, after = split(rec.main(), "advi_info" if advi else "diagnostics")
            assert (before, after) == (plain[advi][0], plain[advi][2]), (o, advi)
            assert read == reads(o, advi, G=G, p=0.05, seed=7, tc=0.7, pooled=False), (o, advi)
            for k in ORDER:
                assert (getattr(res, EXPECT[k][0]) is not None) == o[k], (o, advi, k)
            assert len(w) == n_warnings(o, advi), (o, advi, [str(x.message) for x in w])
    assert valid == {False: 24, True: 16}


@pytest.mark.parametrize("n_checked", [K, 0])
def test_pooled_chains_compose_the_selected_options(rec, n_checked):
    """devices=[0, 0]: the reads are those of the pooled fit (lp=False; its model holds the K checked genes only and, for the
    options that read cells, their exclusions), and without a checked gene the cells are not read"""
    run_pass(rec, {}, n_checked, devices=[0, 0])
    plain = split(rec.main(), "columns" if n_checked else "ppc")
    assert plain[1] == [] and [c[0] for c in plain[2]] == ["fit.close", "model.close"]
    assert plain[0][0] == ("Model", ((n_checked, S), n_checked), canon(dict(lambda_mu_mu=5.612671, device=0, excl=None)))
    blocks = sorted(c for c in rec.calls if c[0] != "MainThread" and c[1] == "fit_nuts")
    assert [dict(b[3])["chain_id_offset"] for b in blocks] == [0, 2] and [dict(b[3])["chains"] for b in blocks] == [2, 1]
    for o in combinations():
        if broken_rules(o, False):
            continue
        res, w = run_pass(rec, o, n_checked, devices=[0, 0])
        before, read, after = split(rec.main(), "columns" if n_checked else "ppc")
        cells = any(o[k] for k in OVER_CELLS)
        small_excl = np.array([1, 5], np.int32)[:2 if n_checked else 0] if cells else None      # cell 20 is gene 5's
        assert before[0] == ("Model", ((n_checked, S), n_checked), canon(dict(lambda_mu_mu=5.612671, device=0, excl=small_excl)))
        assert (before[1:], after) == (plain[0][1:], plain[2]), o
        c = dict(G=n_checked, p=0.05, seed=7, tc=0.7, pooled=True)
        expected = [(n, canon(a), canon(kw)) for k in ORDER if o[k] and not (n_checked == 0 and k in OVER_CELLS)
                    for n, a, kw in [EXPECT[k][2](SimpleNamespace(K=n_checked, r_eff=o["loo_r_eff"], mcse=o["loo_mcse"], **c))]]
        assert read == expected, o
        for k in ORDER:
            assert (getattr(res, EXPECT[k][0]) is not None) == (o[k] and not (n_checked == 0 and k in OVER_CELLS)), (o, k)
        assert len(w) == n_warnings(o, False, n_checked, pooled=True), (o, [str(x.message) for x in w])
        assert all(x.filename.endswith("inference.py") for x in w)


def frame():
    import pandas as pd
    return pd.DataFrame([dict(sample=f"s{s}", transcript=f"g{g}", count=int(COUNTS[g, s]), PValue=0.01 * (g + 1), do_check=g < K,
                              x=float(s % 2), sf=1.0) for g in range(G) for s in range(S)])


@pytest.mark.parametrize("just_discovery", [False, True])
def test_identify_outliers_composes_the_selected_options(rec, just_discovery):
    """both passes get the options that are set and no other, each at its own interval probability (0.05, then 0.005 = 1 % / 4
    samples x 2) and truncation compensation; attrs get <field>_discovery and <field>_test of those options and no other"""
    from ppcseq_amd.methods import identify_outliers
    data = frame()
    kw = dict(formula="~ x", scaling_factor="sf", seed=7, cores=3, just_discovery=just_discovery)
    for o in combinations():
        for advi in (False, True):
            del rec.calls[:]
            bad = broken_rules(o, advi)
            if bad:
                with pytest.raises(ValueError) as e:
                    identify_outliers(data, approximate_posterior_inference=advi, **kw, **o)
                assert str(e.value).split()[0] in bad, (o, advi, str(e.value))
                assert rec.calls == []
                continue
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = identify_outliers(data, approximate_posterior_inference=advi, **kw, **o)
            calls, passes = rec.main(), []
            while any(c[0] == "ppc" for c in calls):
                _, read, calls = split(calls, "advi_info" if advi else "diagnostics")
                passes.append(read)
                calls = calls[1:]
            settings = [dict(p=0.05, tc=1.0)] + ([] if just_discovery else [dict(p=0.005, tc=0.7352941)])
            assert passes == [reads(o, advi, G=G, seed=7, pooled=False, **s) for s in settings], (o, advi)
            names = ["discovery"] if just_discovery else ["discovery", "test"]
            assert sorted(out.attrs) == sorted(([] if just_discovery else ATTRS) + [f"{EXPECT[k][0]}_{n}" for k in ORDER if o[k]
                                                                                   for n in names]), (o, advi)
            assert all(out.attrs[f"{EXPECT[k][0]}_{n}"] is not None for k in ORDER if o[k] for n in names)
            assert len(w) == len(names) * n_warnings(o, advi), (o, advi)


def test_rank_passes_take_no_diagnostics(rec):
    from ppcseq_amd.methods import identify_outliers
    for k in ORDER:
        if EXPECT[k][1] != "advi":
            with pytest.raises(ValueError, match=k + " is not available for passes over several ranks"):
                identify_outliers(frame(), formula="~ x", scaling_factor="sf", approximate_posterior_inference=False, _pass=object(),
                                  **{k: True})
    assert rec.calls == []


def test_a_misspelt_option_is_a_type_error(rec):
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.methods import identify_outliers
    with pytest.raises(TypeError):
        do_inference(COUNTS, X, np.zeros(S), K, check_lo=True)
    with pytest.raises(TypeError):
        identify_outliers(frame(), formula="~ x", scaling_factor="sf", check_loo_interval=True)
    assert rec.calls == []


def test_checked_columns_by_hand():
    from ppcseq_amd.inference import checked_columns
    # the unconstrained vector: 3 hyper-parameters, G intercepts, K alpha_sub_1, (C - 2) K alpha_2, G sigma_raw, 3 more
    assert checked_columns(5, 1, 2).tolist() == [0, 1, 2, 3, 4, 8, 9, 10, 11, 15, 16, 17]
    assert checked_columns(5, 3, 2).tolist() == [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 17, 18, 19]
    assert checked_columns(4, 3, 0).tolist() == [0, 1, 2, 11, 12, 13]
    assert checked_columns(5, 3, 2).dtype == np.int32
