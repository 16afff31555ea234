"""The negative-binomial tail probabilities without a GPU: the CPU build of the kernel's header (ppcseq_amd/csrc/ppcx_nbcdf.h,
tests/ppc_exact_host) against mpmath -- direct summation of the pmf, for y <= 5 000 -- and scipy.stats.nbinom beyond that
(mpmath.betainc does not converge at large parameters), at the edge points of tests/ppc_exact_restate.tails_points: y in
{0, 1, 2, 667, 2 001, 1e5, 2 580 228}, phi in {1e-3, 0.5, 5, 100, 1e5}, mu from 0.01 to 2.6e6 and, for every (y, phi), at the
mean where the continued fraction changes sides and on both sides of it.

Bound (ppc_exact_restate.TAILS_BOUND = 1.52e-9): 4 x the largest error measured, 3.8e-10 -- relative in the smaller tail where it
exceeds 1e-300, absolute in the larger (1.4e-11 over the mpmath points; the largest is at y = 2 580 228 against scipy). Whatever
is measured, the absolute error of either tail stays <= 1e-8, so that the pass-2 threshold 2.4e-4 is resolved to four digits.
The largest number of continued-fraction steps seen is 360 of a cap of 2 048."""
import numpy as np
import pytest

from tests import ppc_exact_restate as R


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


@pytest.fixture(scope="module")
def reference():
    y, mu, phi = R.tails_points()
    eta, le, ge = R.tails_reference(y, mu, phi)
    return dict(y=y, eta=eta, phi=phi, le=le, ge=ge)


def test_tails_against_mpmath_and_scipy(host, reference):
    r = reference
    le, ge, it = R.host_tails(host, r["y"], r["eta"], r["phi"])
    err, ab = R.tails_errors(le, ge, r["le"], r["ge"])
    worst = int(np.argmax(err))
    print("points", err.size, "largest error", err.max(), "at y, mu, phi", r["y"][worst], np.exp(r["eta"][worst]), r["phi"][worst],
          "largest absolute error", ab.max(), "largest step count", it.max())
    assert not np.isnan(le).any() and not np.isnan(ge).any()
    assert err.max() <= R.TAILS_BOUND
    assert ab.max() <= R.TAILS_ABS
    assert it.max() <= 2048, "a point reached the iteration cap"       # kNbCdfMaxIter; 2 049 marks a point that did
    assert np.all(ge[r["y"] == 0] == 1.0)
    assert np.all((le >= 0) & (le <= 1) & (ge >= 0) & (ge <= 1 + 1e-15))


def test_reference_covers_both_sides_of_the_switch(reference):
    r = reference
    a, b = r["phi"], r["y"] + 1.0
    x = r["phi"] / (r["phi"] + np.exp(r["eta"]))
    side = x < (a + 1) / (a + b + 2)
    assert side.sum() > 50 and (~side).sum() > 50
    small = np.minimum(r["le"], r["ge"])
    assert (small > 1e-300).sum() > 150 and ((small > 1e-6) & (small < 1e-2)).sum() >= 10     # pass-2 sized tails are there


def test_invalid_parameters_give_nan(host):
    y = np.array([3, 3, 3, 3, 3, 3])
    eta = np.array([np.nan, np.inf, -np.inf, 1.0, 1.0, 1.0])
    phi = np.array([1.0, 1.0, 1.0, 0.0, -2.0, np.inf])
    le, ge, _ = R.host_tails(host, y, eta, phi)
    assert np.isnan(le).all() and np.isnan(ge).all()
    le, ge, _ = R.host_tails(host, [0, 5], [-800.0, -800.0], [2.0, 2.0])       # e^eta underflows: all the mass at 0
    assert le.tolist() == [1.0, 1.0] and ge.tolist() == [1.0, 0.0]


def test_tails_sum_with_the_pmf(host):
    """P(X <= y) + P(X >= y) = 1 + P(X = y) at random points (scipy's pmf)"""
    from scipy.stats import nbinom
    rng = np.random.default_rng(4)
    mu, phi = np.exp(rng.uniform(-2, 9, 400)), np.exp(rng.uniform(-4, 6, 400))
    y = rng.poisson(mu * rng.uniform(0.2, 3.0, 400)).astype(np.int64)
    le, ge, it = R.host_tails(host, y, np.log(mu), phi)
    pm = nbinom.pmf(y, phi, phi / (phi + mu))
    assert np.abs(le + ge - 1 - pm).max() <= 1e-12
    ref = nbinom.cdf(y, phi, phi / (phi + mu))
    assert np.abs(le - ref).max() <= R.TAILS_BOUND
