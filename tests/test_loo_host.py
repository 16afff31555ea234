"""PSIS-LOO per cell without a GPU: the CPU build of the kernel's header (ppcseq_amd/csrc/ppcx_loo.h, tests/loo_host) against
the numpy restatement (tests/loo_restate.py), the decisions of inference.loo_warnings and the refusals of check_loo."""
import ctypes as C

import numpy as np
import pytest

from tests import loo_restate as L
from tests.host_build import host_lib


def _host_lib():
    return host_lib("loo", {"loo_host_cell": ([C.POINTER(C.c_double), C.c_long, C.c_double, C.c_int, C.POINTER(C.c_double)], None)})


@pytest.fixture(scope="module")
def host():
    return _host_lib()


def host_cell(h, ll, r_eff=1.0, excluded=False):
    ll = np.ascontiguousarray(ll, dtype=np.float64).ravel()
    out = np.zeros(4)
    h.loo_host_cell(ll.ctypes.data_as(C.POINTER(C.c_double)), ll.size, float(r_eff), int(excluded),
                    out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def cases():
    rng = np.random.default_rng(21)
    for n in (20, 25, 224, 1000, 4000):
        yield f"normal ratios n={n}", -L.P.normal_ratios(rng, 3.0, n), 1.0, False
    yield "r_eff 0.3", -L.P.normal_ratios(rng, 2.0, 2000), 0.3, False
    yield "r_eff 2.5", -L.P.normal_ratios(rng, 2.0, 2000), 2.5, False
    yield "gpd 0.7", -np.log(L.P.gpd_sample(rng, 0.7, 1000)), 1.0, False
    yield "heavy tail", -np.log(L.P.gpd_sample(rng, 1.4, 2000)), 1.0, False
    yield "ties in the tail", -rng.poisson(3.0, size=1000).astype(float), 1.0, False
    yield "constant tail", -np.concatenate([rng.normal(size=900), np.full(100, 5.0)]), 1.0, False
    ll = rng.normal(size=1000)
    ll[::7] = np.inf                                            # ratio -Inf: takes no part
    yield "+inf ll", ll, 1.0, False
    ll = rng.normal(size=1000)
    ll[5] = -np.inf
    yield "-inf ll", ll, 1.0, False
    yield "-inf ll excluded", ll, 1.0, True
    ll = rng.normal(size=500)
    ll[9] = np.nan
    yield "nan ll", ll, 1.0, False
    yield "M < 5", rng.normal(size=20), 1.0, False
    yield "excluded", rng.normal(-3.0, 0.7, size=2000), 1.0, True
    yield "far from zero", -L.P.normal_ratios(rng, 5.0, 4000) - 1.0e4, 1.0, False
    yield "negbin-like", -np.abs(rng.standard_t(3, size=3000)) * 4 - 20.0, 1.0, False


def _close(got, ref, tol):
    for g, r in zip(got, ref):
        if not np.isfinite(r):
            assert g == r or (np.isnan(r) and np.isnan(g)), (got, ref)
        else:
            assert abs(g - r) <= tol * max(1.0, abs(r)), (got, ref)


@pytest.mark.parametrize("name,ll,r_eff,excl", list(cases()))
def test_header_matches_restatement(host, name, ll, r_eff, excl):
    _close(host_cell(host, ll, r_eff, excl), L.loo_point(ll, r_eff, excl), 1e-13)


def test_known_fields(host):
    rng = np.random.default_rng(3)
    ll = rng.normal(size=20)                                    # M = 4: raw weights, elpd = -log mean exp(-ll)
    got = host_cell(host, ll)
    assert got[3] == np.inf
    assert abs(got[0] + np.log(np.mean(np.exp(-ll)))) < 1e-13
    lpd = np.log(np.mean(np.exp(ll)))
    assert abs(got[1] - (lpd - got[0])) < 1e-13 and got[2] == -2 * got[0]


# ---- loo_warnings

def test_loo_warnings_threshold():
    from ppcseq_amd.inference import loo_threshold, loo_warnings
    assert loo_threshold(4000) == 0.7 and loo_threshold(2155) == 0.7 and loo_threshold(2154) < 0.7
    assert abs(loo_threshold(1000) - (1 - 1 / 3)) < 1e-15
    assert loo_warnings([0.1, 0.69], 4000) == []
    m = loo_warnings([0.1, 0.71, np.nan], 4000)
    assert len(m) == 1 and m[0].startswith("Some Pareto k diagnostic values are too high.")
    assert loo_warnings([0.66], 1000) == [] and len(loo_warnings([0.67], 1000)) == 1
    assert loo_warnings(np.array([[np.inf]]), 4000) != []
    assert loo_warnings([np.nan], 4000) == [] and loo_warnings([], 4000) == []


def test_check_loo_refuses_advi_and_rank_passes():
    from ppcseq_amd.inference import do_inference
    with pytest.raises(ValueError, match="check_loo"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, approximate_posterior_inference=True,
                     check_loo=True)


def test_identify_outliers_check_loo_refusals():
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="check_loo"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=True, check_loo=True)
    with pytest.raises(ValueError, match="check_loo"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False, check_loo=True,
                          _pass=object())
