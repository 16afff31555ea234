"""The shipped predictive kernels (ppcx_ppc_wave_kernel, ppcx_ppc_kernel in LDS and in the global scratch buffer) held to the
negative binomial itself, through the public entries only: Model.fit_from_draws and Fit.ppc(return_counts_rng=True).

The draws are designed (tests/nb_rng_cases.py): one gene per (mu, phi) point, every row identical, so that a gene's cells share
the distribution and differ only in their stream address. Per path and seed:
  1. a chi-square test of the device's own integers against the exact pmf, p >= 1e-4 per point (the oracle passes it on the
     same layouts in tests/test_nb_rng_distribution.py, so the outcome is known beforehand);
  2. the integers equal the oracle's (ppcx_math.h puts a last-bit disagreement at 1e-13 per draw: none in the 1e7 draws here);
  3. `ci` against numpy on the returned integers: mean and sd to 1e-11 relative, both type-7 quantiles exactly -- on the points
     with 89 % and 99.5 % zeros below maxima beyond 10^4 too, where the bisection runs over a huge range onto ties;
  4. the quantile edges: 1, 2, 63, 64, 65, 4096, 4097 predictive draws with (0.025, 0.975), (0.5, 0.5), (0, 1);
  5. the ends of the range: eta = -750, eta around the guard of rng_exp at 700 and at exp's overflow, phi = 0."""
import numpy as np
import pytest

from tests import nb_rng_cases as cases

pytestmark = pytest.mark.gpu

PATHS = {"wave": (cases.N_WAVE, 0, False), "lds": (cases.N_ROWS, cases.N_LDS, True), "scratch": (cases.N_ROWS, cases.N_SCRATCH, True)}
P_LO, P_HI = 0.025, 0.975


@pytest.fixture(scope="module")
def L():
    from ppcseq_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the product has no CPU fallback")
    return _lib


def _models(L, oracle, variant=False):
    cnt = cases.counts_small(cases.G, cases.S)
    return (L.Model(cnt, cases.X, cases.exposure(variant), cases.K),
            oracle.model(cnt, cases.X, cases.exposure(variant), cases.K, n_threads=16))


def _oracle_counts(oracle, mo, dr, n_gen, resample, seed):
    if resample:
        return oracle.generated_quantities_approx(mo, dr, n_gen, 1.0, seed=seed)
    return oracle.generated_quantities(mo, dr, 1.0, seed=seed)


def _assert_equal_integers(rng, gq, what):
    bad = np.argwhere(rng != gq)
    assert bad.size == 0, (what, len(bad), [(int(j), int(g), int(s), int(rng[j, g, s]), int(gq[j, g, s])) for j, g, s in bad[:8]])


def _check(L, oracle, path, variant):
    rows, n_gen, resample = PATHS[path]
    m, mo = _models(L, oracle, variant)
    dr = cases.designed_draws(rows, variant)
    try:
        f = m.fit_from_draws(dr)
        try:
            for sd in cases.SEEDS:
                ci, rng = f.ppc(1.0, P_LO, P_HI, seed=sd, n_gen=n_gen, resample=resample, return_counts_rng=True)
                worst = 1.0
                for g, cells, mu, phi, (stat, df, p) in cases.pooled_tests(rng, variant):
                    print(f"device {path} variant={variant} gene={g} cells={cells} mu={mu:g} phi={phi:g} seed={sd}: chi2={stat:.2f} df={df} p={p:.4g}")
                    worst = min(worst, p)
                    assert p >= cases.P_MIN, (path, variant, g, cells, sd, stat, df, p)
                print(f"device {path} variant={variant} seed={sd}: smallest p = {worst:.4g}")
                _assert_equal_integers(rng, _oracle_counts(oracle, mo, dr, n_gen, resample, sd), (path, variant, sd))
                cases.assert_summary(ci, rng, P_LO, P_HI, (path, variant, sd))
        finally:
            f.close()
    finally:
        m.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_device_draws_follow_the_negative_binomial(L, oracle, path):
    _check(L, oracle, path, False)


def test_device_draws_with_exposures_and_slopes(L, oracle):
    """eta = exposure + X . T with a non-zero exposure and slope: each kind of cell against its own (mu, phi), computed in fp64
    from the same draws"""
    _check(L, oracle, "wave", True)


def test_quantile_edges(L, oracle):
    """(n - 1) p integral, r = n - 1, one draw (sd is NaN), a last partial turn of the wavefront, the hand-over between the two
    kernels; what the entry refuses, it refuses with PPCX_ERR_ARG (-1)"""
    m, _ = _models(L, oracle)
    try:
        f = m.fit_from_draws(cases.designed_draws(cases.N_WAVE))
        try:
            for n_gen in (1, 2, 63, 64, 65, 4096, 4097):
                for p_lo, p_hi in ((0.025, 0.975), (0.5, 0.5), (0.0, 1.0)):
                    resample = n_gen > cases.N_WAVE
                    if resample:                                           # more draws than rows: only by resampling
                        with pytest.raises(L.PpcxError, match=r"ppcx error -1:"):
                            f.ppc(1.0, p_lo, p_hi, seed=2, n_gen=n_gen)
                    ci, rng = f.ppc(1.0, p_lo, p_hi, seed=2, n_gen=n_gen, resample=resample, return_counts_rng=True)
                    assert rng.shape == (n_gen, cases.K, cases.S)
                    cases.assert_summary(ci, rng, p_lo, p_hi, (n_gen, p_lo, p_hi))
                    if (p_lo, p_hi) == (0.0, 1.0):
                        assert np.array_equal(ci[..., 2], rng.min(0)) and np.array_equal(ci[..., 3], rng.max(0)), n_gen
            for p_lo, p_hi in ((0.6, 0.4), (-0.1, 0.5), (0.5, 1.5)):
                with pytest.raises(L.PpcxError, match=r"ppcx error -1:"):
                    f.ppc(1.0, p_lo, p_hi, seed=2)
        finally:
            f.close()
    finally:
        m.close()


@pytest.mark.parametrize("path", ["wave", "lds"])
def test_ends_of_the_range(L, oracle, path):
    """eta <= -750 gives 0 at every draw; eta from 698.5 to 710 with phi = 1 (fast_exp inside the guard at 700, exp outside, exp's
    overflow) gives the saturated value; sigma_raw = 800 (phi = 0) in every seventh row gives the invalid value at exactly those
    draws, which the quantiles sort last"""
    Ge = len(cases.ENDS_ETA0)
    cnt = cases.counts_small(Ge, cases.S)
    rows, n_gen, resample = (cases.N_WAVE, 0, False) if path == "wave" else (700, cases.N_LDS, True)
    dr = cases.ends_draws(rows)
    m = L.Model(cnt, cases.X, cases.ENDS_EXPO, Ge)
    mo = oracle.model(cnt, cases.X, cases.ENDS_EXPO, Ge, n_threads=16)
    try:
        f = m.fit_from_draws(dr)
        try:
            ci, rng = f.ppc(1.0, P_LO, P_HI, seed=1, n_gen=n_gen, resample=resample, return_counts_rng=True)
        finally:
            f.close()
    finally:
        m.close()
    assert (rng[:, 0] == 0).all()
    assert (rng[:, 1:4] == cases.SATURATED).all()
    gq = _oracle_counts(oracle, mo, dr, n_gen, resample, 1)
    _assert_equal_integers(rng, gq, ("ends", path))
    invalid = rng[:, 4] == cases.INVALID
    if not resample:
        assert np.array_equal(invalid, np.broadcast_to((np.arange(rows) % cases.ENDS_INVALID_EVERY == 0)[:, None], invalid.shape))
    assert 0.10 < invalid.mean() < 0.19 and (rng[:, 4][~invalid] < 10000).all()
    cases.assert_summary(ci, rng, P_LO, P_HI, ("ends", path))
    assert (ci[0, :, :] == 0).all()
    assert (ci[1:4, :, 0] == cases.SATURATED).all() and (ci[1:4, :, 1] == 0).all() and (ci[1:4, :, 2:] == cases.SATURATED).all()
    assert (ci[4, :, 3] == cases.INVALID).all() and (ci[4, :, 2] < 100).all()
