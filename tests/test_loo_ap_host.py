"""PSIS-LOO per cell of an ADVI fit without a GPU: the CPU build of the kernels' header (ppcseq_amd/csrc/ppcx_loo_ap.h,
tests/loo_ap_host) against the numpy restatement (tests/loo_ap_restate.py), the restatement against tests/loo_restate.py where
the approximation is exact and against a conjugate model's analytic leave-one-out density, and the refusals of the two flags."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import loo_ap_cases as cases
from tests import loo_ap_restate as A
from tests import loo_restate as L
from tests import psis_restate as P
from tests.host_build import host_lib


def _host_lib():
    dp = C.POINTER(C.c_double)
    return host_lib("loo_ap", {"loo_ap_host_cell": ([dp, dp, C.c_long, C.c_int, dp], None)})


@pytest.fixture(scope="module")
def host():
    return _host_lib()


def host_cell(h, ll, a, excluded=False):
    ll = np.ascontiguousarray(ll, dtype=np.float64).ravel()
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    out = np.zeros(4)
    dp = C.POINTER(C.c_double)
    h.loo_ap_host_cell(ll.ctypes.data_as(dp), a.ctypes.data_as(dp), ll.size, int(excluded), out.ctypes.data_as(dp))
    return out


def _close(got, ref, tol):
    for g, r in zip(got, ref):
        if not np.isfinite(r):
            assert g == r or (np.isnan(r) and np.isnan(g)), (got, ref)
        else:
            assert abs(g - r) <= tol * max(1.0, abs(r)), (got, ref)


@pytest.mark.parametrize("name,ll,a,excl", list(cases.designed()))
def test_header_matches_restatement(host, name, ll, a, excl):
    got, ref = host_cell(host, ll, a, excl), A.loo_point(ll, a, excl)
    _close(got, ref, 1e-12)
    if name.startswith("normal ll n=20 "):
        assert got[3] == np.inf                                  # M = 4: raw weights
    if name.startswith(("nan", "-inf ll", "+inf ll excluded", "no draw")) and name != "-inf ll excluded":
        assert np.all(np.isnan(got)), name
    elif not name.startswith("far"):
        assert np.all(np.isfinite(got[:3])), name


def test_excluded_cell_has_the_overall_khat(host):
    for name, ll, a, excl in cases.designed():
        if excl and not np.isnan(A.loo_point(ll, a, True)[0]):
            got = host_cell(host, ll, a, True)
            ref = P.khat(a)
            assert got[1] == 0.0 and got[2] == -2.0 * got[0], name
            assert got[3] == ref or abs(got[3] - ref) <= 1e-12 * max(1.0, abs(ref)), (name, got[3], ref)


def test_draws_without_a_ratio_take_no_part(host):
    rng = np.random.default_rng(2)
    ll, a = rng.normal(size=700), rng.normal(size=700)
    drop = np.zeros(700, bool)
    drop[::5] = True
    a_inf = np.where(drop, -np.inf, a)
    for excl in (False, True):
        _close(host_cell(host, ll, a_inf, excl), host_cell(host, ll[~drop], a[~drop], excl), 1e-13)


def test_exact_approximation_gives_plain_loo(host):
    """a constant (g = p up to a factor): the fields of a cell that is not excluded are those of loo::loo at r_eff = 1"""
    rng = np.random.default_rng(6)
    cols = [-L.P.normal_ratios(rng, 3.0, 2000), -np.log(L.P.gpd_sample(rng, 0.7, 1000)), rng.normal(size=25), rng.normal(size=20)]
    for ll in cols:
        for c in (0.0, 1.5):
            ref = L.loo_point(ll)
            _close(A.loo_point(ll, np.full(ll.size, c)), ref, 1e-12)
            _close(host_cell(host, ll, np.full(ll.size, c)), ref, 1e-12)


def test_conjugate_normal_mean():
    """The statistic against an analytic answer, on the restatement. y_i ~ N(mu, 1), i = 1 .. 20, mu ~ N(0, 10^2): the posterior
    p is N(m, s^2), s^2 = 1 / (1 / 100 + 20), m = s^2 sum y; without y_i it is N(m_i, s_i^2), s_i^2 = 1 / (1 / 100 + 19),
    m_i = s_i^2 (sum y - y_i), and the leave-one-out predictive density of y_i is N(y_i; m_i, 1 + s_i^2). The draws come from
    g = N(m + 0.2 s, (1.5 s)^2): wider than every p_i (s_i / s = 1.03), so the ratios p_i / g are bounded and k-hat is below 0.5
    (asserted). Bound: 5 Monte-Carlo standard errors of the self-normalised estimate, formed from the raw weights
    w = exp(a - ll) as tests/test_gpu_loo.py's brute-force test forms it, sd(w) / mean(w) / sqrt(n), with n the number of draws
    (they are independent)."""
    rng = np.random.default_rng(12)
    n_obs, n, tau2 = 20, 4000, 100.0
    y = rng.normal(0.7, 1.0, n_obs)
    s2 = 1.0 / (1.0 / tau2 + n_obs)
    m = s2 * y.sum()
    mg, sg = m + 0.2 * math.sqrt(s2), 1.5 * math.sqrt(s2)
    mu = rng.normal(mg, sg, n)
    log_p = -0.5 * (mu - m) ** 2 / s2 - 0.5 * math.log(2 * math.pi * s2)
    log_g = -0.5 * (mu - mg) ** 2 / sg ** 2 - 0.5 * math.log(2 * math.pi * sg ** 2)
    a = log_p - log_g
    ll = -0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * math.log(2 * math.pi)
    got = A.loo_columns(ll, a)
    s2i = 1.0 / (1.0 / tau2 + n_obs - 1)
    for i in range(n_obs):
        mi = s2i * (y.sum() - y[i])
        exact = -0.5 * (y[i] - mi) ** 2 / (1.0 + s2i) - 0.5 * math.log(2 * math.pi * (1.0 + s2i))
        r = a - ll[:, i]
        w = np.exp(r - r.max())
        se = w.std() / w.mean() / math.sqrt(n)
        print(i, "khat", got[i, 3], "elpd_loo", got[i, 0], "exact", exact, "se", se)
        assert got[i, 3] < 0.5, (i, got[i, 3])
        assert abs(got[i, 0] - exact) <= 5 * se, (i, got[i, 0], exact, se)
    # without the correction (plain PSIS-LOO on draws of g) the answer is off by much more than that: the check can fail
    plain = L.loo_columns(ll)
    assert np.max(np.abs(plain[:, 0] - got[:, 0])) > 0.05


def test_flags_refuse_a_nuts_pass():
    import pandas as pd
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.methods import identify_outliers
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    for flag in ("check_approximation_loo", "check_approximation_loo_intervals"):
        with pytest.raises(ValueError, match=flag + " needs an ADVI pass"):
            do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, approximate_posterior_inference=False,
                         **{flag: True})
        with pytest.raises(ValueError, match=flag + " needs an ADVI pass"):
            identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False, **{flag: True})
