"""The leave-one-out predictive interval per cell without a GPU: the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_loo_predict.h, tests/loo_predict_host) against the numpy restatement (tests/loo_predict_restate.py) on
designed columns and on the inputs of the device's fit test, the restatement's own conventions, and the refusals of
check_loo_intervals.

Tolerances: sums of weights 1e-12 max(1, |ref|); a quantile must lie between the restatement's support points and within
1e-12 max(1, |ref|) + 1e-12 (v* - v-) / (F(v*) - F(v-)). Cells that loo_predict_restate.borderline marks are skipped for lower /
upper only, at most 1 cell in 1 000 per test."""
import ctypes as C

import numpy as np
import pytest

from tests import loo_predict_cases as cases
from tests import loo_predict_restate as R
from tests.host_build import host_lib


def _host_lib():
    dp = C.POINTER(C.c_double)
    return host_lib("loo_predict", {"loo_predict_host_cell": ([dp, C.POINTER(C.c_int32), C.c_long, C.c_int, C.c_double, C.c_int,
                                                               C.c_double, C.c_double, dp], None)})


@pytest.fixture(scope="module")
def host():
    return _host_lib()


def host_cell(h, ll, x, y, r_eff=1.0, excluded=False, p_lo=0.025, p_hi=0.975):
    ll = np.ascontiguousarray(ll, dtype=np.float64).ravel()
    x = np.ascontiguousarray(x, dtype=np.int32).ravel()
    out = np.zeros(6)
    h.loo_predict_host_cell(ll.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_int32)), ll.size, int(y),
                            float(r_eff), int(excluded), float(p_lo), float(p_hi), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


DESIGNED = cases.designed()


@pytest.mark.parametrize("c", DESIGNED, ids=[c["name"] for c in DESIGNED])
def test_header_matches_restatement(host, c):
    kw = dict(r_eff=c["r_eff"], excluded=c["excluded"], p_lo=c["p_lo"], p_hi=c["p_hi"])
    ref = R.point(c["ll"], c["x"], c["y"], **kw)
    got = host_cell(host, c["ll"], c["x"], c["y"], **kw)
    exact = c.get("exact_upper", False)
    skipped = R.check(got, ref, None if exact else c["ll"], c["x"], c["r_eff"], c["p_lo"], c["p_hi"], c["name"])
    assert skipped == 0, "designed columns hold no borderline cell"
    if np.isfinite(got[1]):
        assert got[1] <= got[2] and got[3] <= got[4]


def test_designed_columns_are_what_they_claim():
    by = {c["name"]: c for c in DESIGNED}
    for name in ("nan ll", "-inf ll", "invalid draw", "nan ll excluded"):
        c = by[name]
        assert all(np.isnan(R.point(c["ll"], c["x"], c["y"], excluded=c["excluded"])[k]) for k in R.FIELDS), name
    for name in ("M < 5", "constant tail", "constant column"):
        assert R.point(by[name]["ll"], by[name]["x"], 1)["khat"] == np.inf, name
    for name in ("smooth tail n=1000", "ties inside the tail", "ties straddling the cutoff", "ties from the cutoff up"):
        assert np.isfinite(R.point(by[name]["ll"], by[name]["x"], 1)["khat"]), name
    c = by["v* at the smallest drawn value"]
    assert R.point(c["ll"], c["x"], 0)["support"][0] == (None, int(c["x"].min()))
    c = by["v* at the largest drawn value"]
    assert R.point(c["ll"], c["x"], 0, p_lo=c["p_lo"], p_hi=c["p_hi"])["support"][1][1] == int(c["x"].max())
    c = by["p_lo = 0, p_hi = 1"]
    ref = R.point(c["ll"], c["x"], 0, p_lo=0.0, p_hi=1.0)
    assert ref["lower"] == c["x"].min() and abs(ref["upper"] - c["x"].max()) <= 1e-9 * c["x"].max()
    c = by["all counts equal"]
    ref = R.point(c["ll"], c["x"], 7)
    assert ref["lower"] == ref["upper"] == 7 and ref["pit_lt"] == 0 and abs(ref["pit_le"] - 1) < 1e-12 and abs(ref["mean"] - 7) < 1e-12


def test_tie_rule_decides_the_weights():
    """Among draws tied at the cutoff the highest draw indices are in the tail, in draw order: permuting the counts of the tied
    draws changes the mean, and the header follows the stable sort."""
    c = next(c for c in DESIGNED if c["name"] == "ties straddling the cutoff")
    w, _ = R.weights(c["ll"])
    r = -c["ll"]
    ix = np.argsort(r, kind="stable")
    n, M = r.size, R.L.tail_len(r.size)
    tied = np.nonzero(r == r[ix[n - M - 1]])[0]
    assert tied.size == 10
    assert len(set(np.round(w[tied], 15))) > 2                       # the tied draws carry different weights
    assert np.all(np.diff(w[tied][-5:]) > 0)                          # the last five in draw order are the tail, ascending
    assert np.allclose(w[tied][:5], w[tied][0], rtol=1e-13, atol=0)   # the first five keep the raw weight


def test_excluded_cells_are_type7_quantiles(host):
    rng = np.random.default_rng(8)
    for n, p in ((7, 0.3), (1000, 0.05), (2001, 0.975), (500, 0.5), (999, 0.0017)):
        x = rng.negative_binomial(3, 0.05, n)
        got = host_cell(host, rng.normal(size=n), x, 40, excluded=True, p_lo=p / 2, p_hi=p)
        for q, g in ((p / 2, got[1]), (p, got[2])):
            ref = float(np.quantile(x, q))
            assert abs(g - ref) <= 1e-12 * max(1.0, abs(ref)), (n, q, g, ref)
            assert g == R.type7(x, q)
        assert got[0] == x.sum() / n and np.isnan(got[5])
        assert got[3] == np.sum(x < 40) / n and got[4] == np.sum(x <= 40) / n


def test_fit_inputs_hold_no_borderline_cell(host, oracle):
    """The inputs of the device's fit test (oracle draws, scipy log-likelihood, oracle counts): the header against the
    restatement on all 300 cells, and the restatement alone stays within the cap of borderline cells."""
    f = cases.fit_inputs(oracle)
    d, ll, x = f["d"], f["ll"], f["x"]
    G, S = d["counts"].shape
    skipped = cells = 0
    for g in range(G):
        for s in range(S):
            excl = g * S + s in cases.FIT_EXCL
            y = int(d["counts"][g, s])
            ref = R.point(ll[:, g, s], x[:, g, s], y, excluded=excl)
            got = host_cell(host, ll[:, g, s], x[:, g, s], y, excluded=excl)
            skipped += R.check(got, ref, ll[:, g, s], x[:, g, s], what=(g, s)) > 0
            cells += 1
    assert cells == 300 and skipped <= cells / 1000, skipped


# ---- refusals of check_loo_intervals (no GPU: they come before any device call)

def test_check_loo_intervals_refuses_advi():
    from ppcseq_amd.inference import do_inference
    with pytest.raises(ValueError, match="check_loo_intervals"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, approximate_posterior_inference=True,
                     check_loo_intervals=True)


def test_identify_outliers_check_loo_intervals_refusals():
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="check_loo_intervals"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=True,
                          check_loo_intervals=True)
    with pytest.raises(ValueError, match="check_loo_intervals"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False,
                          check_loo_intervals=True, _pass=object())
