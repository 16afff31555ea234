"""The relative efficiency per cell without a GPU: the CPU build of the kernel's header (ppcseq_amd/csrc/ppcx_reff.h,
tests/reff_host) against the numpy restatement (tests/reff_restate.py), the NaN rules, loose known answers, and the refusals of
loo_r_eff."""
import ctypes as C

import numpy as np
import pytest

from tests import reff_restate as E
from tests.host_build import host_lib


def _host_lib():
    return host_lib("reff", {"reff_host_cell": ([C.POINTER(C.c_double), C.c_int, C.c_int], C.c_double)})


@pytest.fixture(scope="module")
def host():
    return _host_lib()


def host_cell(h, ll):
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    return h.reff_host_cell(ll.ctypes.data_as(C.POINTER(C.c_double)), ll.shape[0], ll.shape[1])


def _close(got, ref, tol):
    if np.isnan(ref):
        assert np.isnan(got), (got, ref)
    else:
        assert abs(got - ref) <= tol * abs(ref), (got, ref)


@pytest.mark.parametrize("name,ll", list(E.seeded_cases()))
def test_header_matches_restatement(host, name, ll):
    ref = E.relative_eff(ll)
    if ll.shape[1] // 2 >= 2:
        assert np.isfinite(ref) and ref > 0, name
        assert E.min_pair_margin(ll) > 1e-9, name                # else rounding could flip the truncation: another seed
    _close(host_cell(host, ll), ref, 1e-12)


@pytest.mark.parametrize("name,ll,expect", list(E.rule_cases()))
def test_rules(host, name, ll, expect):
    got, ref = host_cell(host, ll), E.relative_eff(ll)
    if expect == "nan":
        assert np.isnan(got) and np.isnan(ref), (name, got, ref)
    else:
        assert np.isfinite(got) and got > 0, (name, got)
        _close(got, ref, 1e-12)


def test_underflowing_likelihoods_keep_their_value(host):
    """all ll near -2000: exp(ll) is 0 everywhere, the shifted values give what the column moved up by 2000 gives"""
    rng = np.random.default_rng(5)
    x = -3.0 + E.ar1(rng, 0.5, 4, 64, 0.7)
    a, b = host_cell(host, x - 2000.0), host_cell(host, x)
    assert np.all(np.exp(x - 2000.0) == 0.0) and np.isfinite(a)
    _close(a, b, 1e-12)
    _close(E.relative_eff(x - 2000.0), E.relative_eff(x), 1e-12)


def test_known_answers(host):
    """loose sanity checks, not parity: independent draws are about as efficient as they are many, and an AR(1) series itself
    (v = exp(ll - L) with ll = log of a positive AR(1)-driven value, so that v is the series up to scale) has
    ESS / N near (1 - phi) / (1 + phi)"""
    rng = np.random.default_rng(11)
    r = host_cell(host, rng.normal(-3.0, 0.7, size=(4, 250)))
    assert 0.6 <= r <= 1.6, r
    phi = 0.9
    v = 10.0 + E.ar1(rng, phi, 4, 250)                           # positive: the estimator sees the AR(1) values themselves
    assert v.min() > 0
    r = host_cell(host, np.log(v))
    target = (1 - phi) / (1 + phi)
    assert target / 2 <= r <= target * 2, (r, target)
    _close(r, E.relative_eff(np.log(v)), 1e-12)


def test_loo_r_eff_refusals():
    import pandas as pd
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.methods import identify_outliers
    with pytest.raises(ValueError, match="loo_r_eff"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, loo_r_eff="auto")
    with pytest.raises(ValueError, match="loo_r_eff"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, check_loo=True, loo_r_eff="bogus")
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="loo_r_eff"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False, loo_r_eff="auto")
