"""The fit summary's statistics without a GPU: the numpy restatement (tests/summary_restate.py) on cases with known answers,
the CPU build of the kernel's header (ppcseq_amd/csrc/ppcx_summary.h, tests/summary_host) against it, and the decisions of
inference.convergence_warnings."""
import ctypes as C

import numpy as np
import pytest

from tests import summary_restate as R
from tests.host_build import host_lib


def ar1(rng, M, n, phi):
    x = np.empty((M, n))
    x[:, 0] = rng.normal(size=M) / np.sqrt(1 - phi * phi)
    e = rng.normal(size=(M, n))
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


# ---- cases with known answers, for the restatement and for the header compiled for the CPU (`impl`: the fixture below)

def test_iid_draws_have_ess_near_n(impl):
    x = np.random.default_rng(1).normal(size=(4, 1000))
    s = impl(x)
    N = 4 * 1000
    assert 0.85 * N < s["ess_bulk"] < 1.15 * N
    assert 0.85 * N < s["ess_tail"] < 1.2 * N
    assert s["rhat"] < 1.01


def test_ar1_ess_matches_theory(impl):
    phi = 0.9
    x = ar1(np.random.default_rng(2), 4, 5000, phi)
    s = impl(x)
    expect = 4 * 5000 * (1 - phi) / (1 + phi)
    assert 0.75 * expect < s["ess_bulk"] < 1.3 * expect, (s["ess_bulk"], expect)


def test_one_shifted_chain_raises_rhat(impl):
    x = np.random.default_rng(3).normal(size=(4, 250))
    assert impl(x)["rhat"] < 1.05
    x[2] += 1.0
    assert impl(x)["rhat"] > 1.05


def test_odd_n_drops_the_middle_draw(impl):
    rng = np.random.default_rng(4)
    x = rng.normal(size=(4, 251))
    x[:, 125] = 50.0 + rng.normal(size=4)                 # the middle draws: in the plain summary, not in the split chains
    odd = impl(x)
    even = impl(np.delete(x, 125, axis=1))
    for k in ("rhat", "ess_bulk", "ess_tail"):
        assert odd[k] == even[k], k
    assert odd["mean"] > even["mean"] and odd["sd"] > even["sd"]          # the plain summary keeps them


def test_heavy_ties(impl):
    x = np.random.default_rng(8).integers(0, 3, size=(4, 300)).astype(float)     # three values: most draws tie
    s = impl(x)
    assert s["q50"] == 1.0 and np.isfinite(s["rhat"]) and s["rhat"] < 1.05
    assert 0.5 * 1200 < s["ess_bulk"] < 1.5 * 1200


def test_constant_and_non_finite_columns(impl):
    c = impl(np.full((4, 100), 2.5))
    assert c["mean"] == 2.5 and c["sd"] == 0.0 and c["q50"] == 2.5
    assert all(np.isnan(c[k]) for k in ("rhat", "ess_bulk", "ess_tail"))
    x = np.random.default_rng(5).normal(size=(4, 100))
    x[1, 7] = np.inf
    assert all(np.isnan(impl(x)[k]) for k in R.FIELDS)


# ---- the header, compiled for the CPU

@pytest.fixture(scope="module")
def host():
    return _host_lib()


@pytest.fixture(params=["restatement", "header"])
def impl(request):
    if request.param == "restatement":
        return R.summary_column
    h = _host_lib()
    return lambda x: host_column(h, x)[0]


def _host_lib():
    dp = C.POINTER(C.c_double)
    return host_lib("summary", {"summary_host_column": ([dp, C.c_int, C.c_int, dp, dp], None),
                                "summary_host_ndtri": ([C.c_double], C.c_double)})


def host_column(h, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    M, n = x.shape
    out = np.zeros(8)
    rk = np.zeros(max(2 * M * (n // 2), 1))
    dp = C.POINTER(C.c_double)
    h.summary_host_column(x.ctypes.data_as(dp), M, n, out.ctypes.data_as(dp), rk.ctypes.data_as(dp))
    return dict(zip(R.FIELDS, out)), rk


def cases():
    rng = np.random.default_rng(11)
    yield "iid 4x250", rng.normal(size=(4, 250))
    yield "iid 8x251", rng.normal(1.0, 3.0, size=(8, 251))
    yield "ar1 4x400", ar1(rng, 4, 400, 0.7)
    yield "shifted", rng.normal(size=(4, 100)) + np.array([[0.0], [0.0], [2.0], [0.0]])
    yield "ties", rng.poisson(2.0, size=(4, 200)).astype(float)
    yield "heavy ties", rng.integers(0, 3, size=(3, 81)).astype(float)
    yield "one chain", rng.standard_t(3, size=(1, 300))
    yield "64 chains", rng.normal(size=(64, 5))
    yield "skewed", np.exp(rng.normal(size=(4, 250)))


@pytest.mark.parametrize("name,x", list(cases()))
def test_header_matches_restatement(host, name, x):
    got, rk = host_column(host, x)
    ref = R.summary_column(x)
    for k in ("q05", "q50", "q95"):
        assert got[k] == ref[k], (name, k)
    if ref["ranks"] is not None:
        assert np.array_equal(rk[:ref["ranks"].size], ref["ranks"]), name
    for k in ("mean", "sd", "rhat", "ess_bulk", "ess_tail"):
        if np.isnan(ref[k]):
            assert np.isnan(got[k]), (name, k)
        else:
            assert abs(got[k] - ref[k]) <= 1e-12 * max(abs(ref[k]), 1e-300), (name, k, got[k], ref[k])


def test_header_nan_rules(host):
    assert all(np.isnan(host_column(host, np.full((4, 50), 1.0))[0][k]) for k in ("rhat", "ess_bulk", "ess_tail"))
    x = np.random.default_rng(6).normal(size=(4, 50))
    x[0, 0] = np.nan
    assert all(np.isnan(v) for v in host_column(host, x)[0].values())
    x = np.random.default_rng(7).normal(size=(4, 3))                     # n' = 1
    got = host_column(host, x)[0]
    assert np.isfinite(got["mean"]) and np.isnan(got["rhat"]) and np.isnan(got["ess_bulk"])


def test_header_ndtri(host):
    from scipy.special import ndtri
    for p in np.concatenate([np.linspace(1e-6, 1 - 1e-6, 1001), [1e-12, 0.02425, 0.5, 1 - 0.02425]]):
        ref = ndtri(p)
        assert abs(host.summary_host_ndtri(p) - ref) <= 1e-13 * max(abs(ref), 1.0), p


# ---- convergence_warnings

def fake(rhat, bulk, tail):
    return dict(rhat=np.asarray(rhat, float), ess_bulk=np.asarray(bulk, float), ess_tail=np.asarray(tail, float))


def test_convergence_warnings_decisions():
    from ppcseq_amd.inference import convergence_warnings
    assert convergence_warnings(fake([1.0, 1.04], [500, 900], [450, 401]), chains=4) == []
    m = convergence_warnings(fake([1.0, 1.23], [500, 900], [450, 401]), chains=4)
    assert len(m) == 1 and m[0].startswith("The largest R-hat is 1.23, indicating chains have not mixed.")
    m = convergence_warnings(fake([1.0, 1.0], [399, 900], [450, 401]), chains=4)
    assert len(m) == 1 and m[0].startswith("Bulk Effective Samples Size (ESS) is too low, ")
    m = convergence_warnings(fake([1.0, 1.0], [500, 900], [450, 399]), chains=4)
    assert len(m) == 1 and m[0].startswith("Tail Effective Samples Size (ESS) is too low, ")
    m = convergence_warnings(fake([1.2, np.nan], [10, np.nan], [10, np.nan]), chains=8)
    assert [s.split(" ")[0] for s in m] == ["The", "Bulk", "Tail"]
    assert convergence_warnings(fake([np.nan], [np.nan], [np.nan]), chains=4) == []     # NaN: no variance, nothing to report
    assert convergence_warnings(fake([], [], []), chains=4) == []


def test_check_convergence_refuses_advi():
    from ppcseq_amd.inference import do_inference
    with pytest.raises(ValueError):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, approximate_posterior_inference=True,
                     check_convergence=True)


def test_identify_outliers_check_convergence_needs_nuts():
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="check_convergence"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=True, check_convergence=True)
