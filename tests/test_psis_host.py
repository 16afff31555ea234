"""The Pareto-k diagnostic without a GPU: the numpy restatement (tests/psis_restate.py) and the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_psis.h, tests/psis_host) on cases with known answers, the header against the restatement, and the
decisions of inference.approximation_warnings."""
import ctypes as C

import numpy as np
import pytest

from tests import psis_restate as R
from tests.host_build import host_lib


def _host_lib():
    return host_lib("psis", {"psis_host_khat": ([C.POINTER(C.c_double), C.c_long], C.c_double)})


def host_khat(h, v):
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    return h.psis_host_khat(v.ctypes.data_as(C.POINTER(C.c_double)), v.size)


@pytest.fixture(scope="module")
def host():
    return _host_lib()


@pytest.fixture(params=["restatement", "header"])
def impl(request):
    if request.param == "restatement":
        return R.khat
    h = _host_lib()
    return lambda v: host_khat(h, v)


# ---- cases with known answers, for the restatement and for the header compiled for the CPU

@pytest.mark.parametrize("k", [0.3, 0.5, 0.9])
def test_gpd_samples_recover_the_shape(impl, k):
    rng = np.random.default_rng(0)
    for kk in (0.3, 0.5, 0.9):                  # one stream for the three shapes, in this order
        r = np.log(R.gpd_sample(rng, kk, 100_000))
        if kk == k:
            break
    assert abs(impl(r) - k) <= 0.1, (k, impl(r))


def test_normal_ratios_recover_the_shape_and_rise(impl):
    got = []
    for s2 in (2.0, 4.0, 10.0):
        kh = impl(R.normal_ratios(np.random.default_rng(0), s2, 100_000))
        assert abs(kh - (1.0 - 1.0 / s2)) <= 0.1, (s2, kh)
        got.append(kh)
    assert got[0] < got[1] < got[2], got


def test_shift_invariance(impl):
    r = R.normal_ratios(np.random.default_rng(3), 4.0, 5000)
    base = impl(r)
    for c in (-700.0, -3.5, 12.25, 900.0):
        assert abs(impl(r + c) - base) <= 1e-9, c


def test_short_and_constant_tails_are_inf(impl):
    rng = np.random.default_rng(4)
    assert impl(rng.normal(size=20)) == np.inf                  # M = 4
    assert np.isfinite(impl(rng.normal(size=25)))               # M = 5
    v = rng.normal(size=1000)
    v[np.argsort(v)[-95:]] = 3.0                                # the 95 tail values tie
    assert impl(v) == np.inf
    assert impl(np.full(500, -1.25)) == np.inf


def test_minus_inf_ratios_take_no_part(impl):
    rng = np.random.default_rng(5)
    r = rng.normal(size=1000)
    with_inf = np.concatenate([r[:400], np.full(37, -np.inf), r[400:]])
    assert impl(with_inf) == impl(r)
    v = np.full(30, -np.inf)
    v[:20] = rng.normal(size=20)
    assert impl(v) == np.inf                                    # 20 finite values: M = 4


def test_non_finite_entries_give_nan(impl):
    r = np.random.default_rng(6).normal(size=300)
    for bad in (np.nan, np.inf):
        v = r.copy()
        v[123] = bad
        assert np.isnan(impl(v)), bad
    theta = np.random.default_rng(7).normal(size=300)
    theta[5] = np.nan
    assert np.isnan(impl(R.column_values(theta, r)))
    theta[5] = np.inf
    assert np.isnan(impl(R.column_values(theta, r)))


# ---- the header against the restatement

def cases():
    rng = np.random.default_rng(11)
    for n in (20, 224, 225, 1000, 100_000):
        yield f"normal ratios n={n}", R.normal_ratios(rng, 3.0, n)
    yield "gpd 0.7 n=1000", np.log(R.gpd_sample(rng, 0.7, 1000))
    yield "light tail", rng.normal(size=2000) * 0.1
    yield "ties", rng.poisson(3.0, size=1000).astype(float)
    yield "constant tail", np.concatenate([rng.normal(size=900), np.full(100, 5.0)])
    r = rng.normal(size=1000)
    r[::7] = -np.inf
    yield "-inf ratios", r
    theta = rng.normal(2.0, 0.3, size=1000)
    yield "parameter column", R.column_values(theta, R.normal_ratios(rng, 2.0, 1000))
    theta[17] = np.nan
    yield "non-finite column", R.column_values(theta, rng.normal(size=1000))
    yield "far from zero", R.normal_ratios(rng, 5.0, 4000) - 1.0e4


@pytest.mark.parametrize("name,v", list(cases()))
def test_header_matches_restatement(host, name, v):
    got, ref = host_khat(host, v), R.khat(v)
    if not np.isfinite(ref):
        assert got == ref or (np.isnan(ref) and np.isnan(got)), (name, got, ref)
    else:
        assert abs(got - ref) <= 1e-13 * max(abs(ref), 1e-300), (name, got, ref)


def test_tail_lengths():
    assert [R.tail_len(n) for n in (20, 21, 224, 225, 1000, 100_000)] == [4, 5, 45, 45, 95, 949]


# ---- approximation_warnings

def test_approximation_warnings_decisions():
    from ppcseq_amd.inference import approximation_warnings
    assert approximation_warnings([0.2, 0.69]) == []
    m = approximation_warnings([0.3, 0.71])
    assert len(m) == 1 and m[0].startswith("Pareto k diagnostic value is 0.71. Resampling is unreliable.")
    m = approximation_warnings([1.01, 0.5])
    assert len(m) == 1 and m[0].startswith("Pareto k diagnostic value is 1.01. Resampling is disabled.")
    m = approximation_warnings([np.inf])
    assert len(m) == 1 and m[0].startswith("Pareto k diagnostic value is Inf. Resampling is disabled.")
    assert approximation_warnings([np.nan]) == []               # a column with a non-finite draw: nothing to report
    assert approximation_warnings([]) == []


def test_check_approximation_refuses_nuts():
    from ppcseq_amd.inference import do_inference
    with pytest.raises(ValueError, match="check_approximation"):
        do_inference(np.ones((3, 4), np.int32), np.ones((4, 1)), np.zeros(4), 1, approximate_posterior_inference=False,
                     check_approximation=True)


def test_identify_outliers_check_approximation_needs_advi():
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="check_approximation"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False,
                          check_approximation=True)
