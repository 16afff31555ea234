"""The Monte-Carlo standard error of elpd_loo and the PSIS n_eff per cell without a GPU: the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_loo.h steps 5 - 8, tests/loo_mcse_host) against the numpy restatement (tests/loo_mcse_restate.py), known
answers, loo's own frame, and the host logic of the Python layer (pareto_k_table, mcse_elpd_loo_total, the loo_mcse argument).

mcse_elpd_loo is compared relative to the restated value itself: the largest relative difference between the CPU build and the
restatement on the designed columns is 1.65e-14 (tests/loo_mcse_cases.py MCSE_MEASURED); the bound, here and on the device, is
ten times that, 1.65e-13."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import loo_mcse_cases as K
from tests import loo_mcse_restate as R
from tests import loo_restate as L
from tests.host_build import ROOT, host_lib


def _host_lib():
    return host_lib("loo_mcse", {"loo_mcse_host_cell": ([C.POINTER(C.c_double), C.c_long, C.c_double, C.c_int, C.POINTER(C.c_double)],
                                                        None)})


@pytest.fixture(scope="module")
def host():
    return _host_lib()


def host_cell(h, ll, r_eff=1.0, excluded=False):
    ll = np.ascontiguousarray(ll, dtype=np.float64).ravel()
    out = np.zeros(6)
    h.loo_mcse_host_cell(ll.ctypes.data_as(C.POINTER(C.c_double)), ll.size, float(r_eff), int(excluded),
                         out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def host_columns(h, ll, r_eff, excl):
    n = ll.shape[1]
    r_eff = np.ones(n) if r_eff is None else r_eff
    return np.array([host_cell(h, ll[:, i], r_eff[i], bool(excl[i])) for i in range(n)])


@pytest.mark.parametrize("which", ["designed", "small"])
@pytest.mark.parametrize("with_r_eff", [False, True])
def test_header_matches_restatement(host, which, with_r_eff):
    ll, excl, r_eff = K.designed() if which == "designed" else K.small()
    got = host_columns(host, ll, r_eff if with_r_eff else None, excl)
    K.compare(got, K.reference(which, with_r_eff), (which, with_r_eff))
    if which == "small" and not with_r_eff:
        assert got[0, 3] == np.inf                               # M = 4: raw weights
        w = np.exp(-ll[:, 0] - L.logsumexp(-ll[:, 0]))
        assert abs(got[0, 5] - 1.0 / np.sum(w * w)) <= 1e-12 * got[0, 5]


def test_first_four_fields_are_those_without_mcse(host):
    """loo_cell_host with and without the two fields gives the same bits (the kernel's flag promises the same)"""
    from tests.test_loo_host import _host_lib as four_lib, host_cell as four_cell
    h4 = four_lib()
    ll, excl, r_eff = K.designed()
    for i in range(ll.shape[1]):
        for re in (1.0, float(r_eff[i])):
            six = host_cell(host, ll[:, i], re, bool(excl[i]))
            assert np.array_equal(six[:4], four_cell(h4, ll[:, i], re, bool(excl[i])), equal_nan=True), (i, re)


def test_known_answers(host):
    ll, excl, r_eff = K.designed()
    # uniform weights: n_eff = N r_eff exactly
    for re in (1.0, 0.37, float(r_eff[-1])):
        assert host_cell(host, ll[:, -1], re, True)[5] == 3000 * re
    col = ll[:, 5]                                               # every ninth draw takes no part
    assert host_cell(host, col, 0.8, True)[5] == int(np.sum(col != np.inf)) * 0.8
    # a constant column: c = 0, mcse = 0, and every weight 1 / N
    for excluded in (False, True):
        for n in (3000, 777, 20):
            got = host_cell(host, np.full(n, -2.5), 1.3, excluded)
            assert got[4] == 0.0, (n, excluded, got)
            assert abs(got[5] - n * 1.3) <= 1e-12 * n * 1.3
    # NaN cells are NaN in both
    assert np.all(np.isnan(host_cell(host, ll[:, 6])[4:])) and np.all(np.isnan(host_cell(host, ll[:, 7])[4:]))
    assert np.all(np.isfinite(host_cell(host, ll[:, 6], 1.0, True)[4:]))     # ll = -Inf in an excluded cell is a value
    # the bounds of n_eff: between r_eff (one draw carries everything) and N r_eff
    for i in range(5):
        got = host_cell(host, ll[:, i], r_eff[i])
        assert r_eff[i] <= got[5] <= 3000 * r_eff[i] and got[4] > 0


def test_loo_frame_equals_shifted_frame(host):
    """loo's E + sd z on exp(ll) against log1p(c z) on columns that do not underflow: 1e-12 relative, for the restatement
    and for the CPU build"""
    ll, excl, r_eff = K.designed()
    for i in (0, 1, 2, 3, 4):
        for re in (1.0, float(r_eff[i])):
            ref = R.mcse_loo_frame(ll[:, i], re)
            assert abs(R.mcse_point(ll[:, i], re)[4] - ref) <= 1e-12 * ref, (i, re)
            assert abs(host_cell(host, ll[:, i], re)[4] - ref) <= K.MCSE_RTOL * ref, (i, re)
    far = ll[:, 1] - 2000.0                                      # exp(ll) underflows: the shifted frame stays defined
    a, b = host_cell(host, far, 1.0), host_cell(host, ll[:, 1], 1.0)
    assert abs(a[4] - b[4]) <= K.MCSE_RTOL * b[4] and abs(a[5] - b[5]) <= 1e-9 * b[5]


def test_scores_and_truncation(host):
    """step 7 alone: at least 500 of the 1 000 scores take part however large c is; c = 0 gives 0"""
    z = R.blom_scores()
    assert z.size == 1000 and np.sum(z > 0) == 500 and abs(z[0] + z[-1]) < 1e-12
    assert R.mcse_from_c(0.0) == 0.0
    big = R.mcse_from_c(1e6)
    assert np.isfinite(big) and big > 0
    # a column whose c exceeds 1 / z_max, so that scores are dropped: one dominant draw among few
    ll = np.concatenate([np.full(40, -1.0), [-9.0]])
    got, ref = host_cell(host, ll), R.mcse_point(ll)
    assert ref[4] > 0.3
    assert abs(got[4] - ref[4]) <= K.MCSE_RTOL * ref[4] and abs(got[5] - ref[5]) <= 1e-12 * ref[5]


# ---- the Python layer's host logic

def _loo_dict():
    khat = np.array([[0.1, 0.5, 0.69, 0.71], [0.9, 1.0, 1.2, np.nan], [np.inf, -0.2, 0.3, 2.0]])
    excluded = np.zeros_like(khat, bool)
    excluded[1, 3] = True                                        # the NaN k-hat: an excluded cell
    excluded[2, 3] = True                                        # excluded cells are not counted, whatever they hold
    n_eff = np.arange(1.0, 13.0).reshape(3, 4) * 100
    mcse = np.full_like(khat, 0.01)
    return dict(khat=khat, excluded=excluded, n_eff=n_eff, mcse_elpd_loo=mcse, n_draws=4000)


def test_pareto_k_table():
    from ppcseq_amd.inference import pareto_k_table
    d = _loo_dict()
    t = pareto_k_table(d)
    assert t["threshold"] == 0.7
    good, bad, very = t["bins"]
    assert (good["lower"], good["upper"]) == (-np.inf, 0.7) and (bad["lower"], bad["upper"]) == (0.7, 1.0)
    assert (very["lower"], very["upper"]) == (1.0, np.inf)
    # ten cells counted: 0.1 0.5 0.69 -0.2 0.3 | 0.71 0.9 1.0 | 1.2 Inf
    assert [b["count"] for b in t["bins"]] == [5, 3, 2]
    assert [b["pct"] for b in t["bins"]] == [50.0, 30.0, 20.0]
    assert [b["min_n_eff"] for b in t["bins"]] == [100.0, 400.0, 700.0]
    del d["n_eff"]
    assert all(np.isnan(b["min_n_eff"]) for b in pareto_k_table(d)["bins"])
    d = _loo_dict()
    d["khat"] = np.minimum(d["khat"], 0.2)
    t = pareto_k_table(d)
    assert [b["count"] for b in t["bins"]] == [10, 0, 0] and np.isnan(t["bins"][1]["min_n_eff"])
    assert t["bins"][0]["min_n_eff"] == 100.0
    d["n_draws"] = 1000                                          # the threshold follows the draws
    assert abs(pareto_k_table(d)["threshold"] - (1 - 1 / 3)) < 1e-15


def test_mcse_total():
    from ppcseq_amd.inference import loo_mcse_total
    d = _loo_dict()
    assert np.isnan(loo_mcse_total(d))                           # k-hats above 0.7 among the cells counted
    d["khat"] = np.where(np.isnan(d["khat"]), np.nan, np.minimum(d["khat"], 0.7))
    d["khat"][2, 3] = 5.0                                        # an excluded cell's k-hat is not looked at
    assert abs(loo_mcse_total(d) - np.sqrt(10 * 0.01 ** 2)) < 1e-15
    d["khat"][0, 0] = 0.70001
    assert np.isnan(loo_mcse_total(d))
    d["khat"][0, 0] = 0.68
    d["n_draws"] = 1000                                          # threshold 2/3
    assert np.isnan(loo_mcse_total(d))


def test_loo_mcse_needs_check_loo():
    import pandas as pd
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.methods import identify_outliers
    with pytest.raises(ValueError, match="loo_mcse needs check_loo"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, loo_mcse=True)
    with pytest.raises(ValueError, match="loo_mcse needs check_loo"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, check_loo_intervals=True, loo_mcse=True)
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="loo_mcse needs check_loo"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False, loo_mcse=True)


def test_binding_names_the_fields():
    from ppcseq_amd import _lib
    assert _lib.LOO_MCSE_FIELDS == R.FIELDS and _lib.LOO_MCSE_FIELDS[:4] == _lib.LOO_FIELDS
    hdr = open(os.path.join(ROOT, "include", "ppcx.h")).read()
    assert "#define PPCX_LOO_MCSE_FIELDS 6" in hdr and "ppcx_fit_loo_mcse" in _lib.EXPORTS
