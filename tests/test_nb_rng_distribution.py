"""The predictive sampler against the negative binomial itself, without a GPU.

Every other test of nb2_log_rng compares two statements of one algorithm (the product's ppcx_math.h and oracle/ppc_oracle.c): a
wrong constant, branch or stream offset on both sides would pass. Here the integers of both go through a chi-square test against
the exact pmf of scipy.stats.nbinom at the designed points of tests/nb_rng_cases.py -- each point is there for a regime of the
sampler (Knuth / PTRS, the a < 1 boost, the saturation at 2^30, the Poisson limit) -- at the seeds 1, 2, 3 fixed in advance,
200 000 draws per point, and must reach p >= 1e-4 every time.

The second half runs the oracle through generated_quantities / generated_quantities_approx on exactly the models, draws and
cell layout of tests/test_gpu_nb_rng.py, so that what the device has to return (it must equal these integers) is known to pass
the same test before a GPU is visited.

That the test can fail was shown by mutating a scratch copy of ppcx_math.h one change at a time (no boost factor, d = a - 0.3,
PTRS + 0.43 -> - 0.07, the Box-Muller spare taken from the cosine too, the Poisson stream on the gamma stream's counter): each
is rejected at one point at least (the weakest, PTRS, with p = 1e-6 at (10.5, 1e5); at 20 000 draws per point it and the spare
passed, hence 200 000); DESIGN.md (section 1, a9) keeps the table."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import nb_rng_cases as cases
from tests.emul_util import P


@pytest.fixture(scope="module")
def oracle_points(oracle):
    """{seed: [n, 16]} the oracle's draws 0 .. n - 1 of cell = point index: one gene per point, one sample, identical rows"""
    Gp = len(cases.POINTS)
    o = cases.offsets(Gp, 1, Gp)
    u = np.zeros(o["D"])
    for g, (mu, phi) in enumerate(cases.POINTS):
        u[o["intercept"] + g] = math.log(mu)
        u[o["sigma_raw"] + g] = -math.log(phi)
    m = oracle.model(np.zeros((Gp, 1), np.int32), np.ones((1, 1)), np.zeros(1), Gp, n_threads=4)
    dr = np.tile(u, (cases.N_CPU, 1))
    return {sd: oracle.generated_quantities(m, dr, 1.0, seed=sd)[:, :, 0] for sd in cases.SEEDS}


def test_generated_quantities_addresses_cell_and_draw(oracle, oracle_points):
    """the layout above is what it claims: column g, row j is nb2_log_rng(ln mu_g, phi_g, seed, cell g, draw j)"""
    for g, (mu, phi) in enumerate(cases.POINTS):
        phi_d = math.exp(-(-math.log(phi)))                    # as generated_quantities forms it from sigma_raw
        for j in (0, 1, 4095, cases.N_CPU - 1):
            assert oracle_points[2][j, g] == oracle.nb2_log_rng(math.log(mu), phi_d, 2, g, j), (g, j)


@pytest.mark.parametrize("point", range(len(cases.POINTS)), ids=[f"mu{m:g}-phi{p:g}" for m, p in cases.POINTS])
def test_oracle_draws_follow_the_negative_binomial(oracle_points, point):
    mu, phi = cases.POINTS[point]
    for sd in cases.SEEDS:
        stat, df, p = cases.chi2_gof(oracle_points[sd][:, point], mu, phi)
        print(f"oracle mu={mu:g} phi={phi:g} seed={sd}: chi2={stat:.2f} df={df} p={p:.4g}")
        assert p >= cases.P_MIN, (mu, phi, sd, stat, df, p)


@pytest.mark.parametrize("point", range(len(cases.POINTS)), ids=[f"mu{m:g}-phi{p:g}" for m, p in cases.POINTS])
def test_emulated_draws_follow_the_negative_binomial(emul, oracle_points, point):
    """the product's ppcx_math.h compiled for the host: the same test, and the oracle's integers"""
    emul.emul_nb2_log_rng_draws.argtypes = [C.c_double, C.c_double, C.c_ulonglong, C.c_uint, C.c_int, C.POINTER(C.c_int32)]
    mu, phi = cases.POINTS[point]
    phi_d = math.exp(-(-math.log(phi)))
    for sd in cases.SEEDS:
        x = np.zeros(cases.N_CPU, np.int32)
        assert emul.emul_nb2_log_rng_draws(math.log(mu), phi_d, sd, point, cases.N_CPU, P(x, C.c_int32)) == 0
        stat, df, p = cases.chi2_gof(x, mu, phi)
        print(f"emulation mu={mu:g} phi={phi:g} seed={sd}: chi2={stat:.2f} df={df} p={p:.4g}")
        assert p >= cases.P_MIN, (mu, phi, sd, stat, df, p)
        assert np.array_equal(x, oracle_points[sd][:, point]), (mu, phi, sd)


def test_helper_rejects_a_wrong_distribution_and_accepts_numpy():
    """the helper itself: numpy's negative binomial passes, a dispersion off by 30 % or a mean off by 15 % does not"""
    g = np.random.default_rng(5)
    for mu, phi in ((3.0, 0.5), (50.0, 4.0), (1e4, 1e4)):
        x = g.negative_binomial(phi, phi / (phi + mu), 20000)
        assert cases.chi2_gof(x, mu, phi)[2] >= cases.P_MIN
        assert cases.chi2_gof(x, mu, phi * 1.3)[2] < 1e-6 or phi > 1e3          # at phi = 1e4 the dispersion hardly shows
        assert cases.chi2_gof(x, mu * 1.15, phi)[2] < 1e-6
    # the saturated point: the censored mass is the last bin's
    mu, phi = 3e8, 5.0
    lam = g.gamma(phi, mu / phi, 200000)
    x = np.where(lam < 2.0 ** 30, g.poisson(np.minimum(lam, 2.0 ** 30)), cases.SATURATED)
    stat, df, p = cases.chi2_gof(x, mu, phi)
    assert p >= cases.P_MIN and df >= 30
    assert cases.chi2_gof(np.minimum(x, 2 ** 29), mu, phi)[2] < 1e-6


# ---- the layouts of tests/test_gpu_nb_rng.py on the oracle ---------------------------------------------------------------------------
def _oracle_model(oracle, variant):
    return oracle.model(cases.counts_small(cases.G, cases.S), cases.X, cases.exposure(variant), cases.K, n_threads=8)


@pytest.mark.parametrize("variant", [False, True], ids=["plain", "exposures-and-slopes"])
def test_oracle_passes_on_the_wavefront_layout(oracle, variant):
    mo = _oracle_model(oracle, variant)
    dr = cases.designed_draws(cases.N_WAVE, variant)
    for sd in cases.SEEDS:
        gq = oracle.generated_quantities(mo, dr, 1.0, seed=sd)
        for g, cells, mu, phi, (stat, df, p) in cases.pooled_tests(gq, variant):
            print(f"wave variant={variant} gene={g} cells={cells} mu={mu:g} phi={phi:g} seed={sd}: chi2={stat:.2f} df={df} p={p:.4g}")
            assert p >= cases.P_MIN, (variant, g, cells, sd, stat, df, p)


@pytest.mark.parametrize("n_gen", [cases.N_LDS, cases.N_SCRATCH])
def test_oracle_passes_on_the_resampled_layouts(oracle, n_gen):
    mo = _oracle_model(oracle, False)
    dr = cases.designed_draws(cases.N_ROWS)
    for sd in cases.SEEDS:
        gq = oracle.generated_quantities_approx(mo, dr, n_gen, 1.0, seed=sd)
        for g, cells, mu, phi, (stat, df, p) in cases.pooled_tests(gq):
            print(f"n_gen={n_gen} gene={g} mu={mu:g} phi={phi:g} seed={sd}: chi2={stat:.2f} df={df} p={p:.4g}")
            assert p >= cases.P_MIN, (n_gen, g, sd, stat, df, p)
        if n_gen == cases.N_SCRATCH:                                  # (3e8, 5): 9e-5 of the mass lies above 2^30
            assert (gq[:, 13] == cases.SATURATED).sum() >= 5 and gq[:, 13].max() == cases.SATURATED


def test_numpy_summary_agrees_with_the_oracle_summary(oracle):
    """tests/nb_rng_cases.py summary_numpy (what the GPU tests hold `ci` to) against oracle.summarise on the designed draws: the
    same quantiles bit for bit, also on 89 % and 99.5 % zeros below maxima beyond 10^4"""
    mo = _oracle_model(oracle, False)
    gq = oracle.generated_quantities(mo, cases.designed_draws(cases.N_WAVE), 1.0, seed=1)
    for p_lo, p_hi in ((0.025, 0.975), (0.5, 0.5), (0.0, 1.0), (0.0005, 0.9995)):
        ref = oracle.summarise(gq, p_lo, p_hi)
        got = cases.summary_numpy(gq, p_lo, p_hi)
        assert np.array_equal(ref[..., 2:], got[..., 2:]), (p_lo, p_hi)
        assert np.max(np.abs(ref[..., :2] - got[..., :2]) / np.abs(ref[..., :2])) < 1e-12
    assert (gq[:, 6] == 0).mean() > 0.85 and gq[:, 6].max() > 1e4     # (1e3, 0.01), (200, 3.4e-4): ties below a huge range
    assert (gq[:, 7] == 0).mean() > 0.99 and gq[:, 7].max() > 1e4


def test_ends_of_the_range_on_the_oracle(oracle):
    """the model of the ends (tests/nb_rng_cases.py ENDS_*): zeros at eta <= -750, the saturated value from eta = 698.5 up,
    the invalid value in every seventh row of the last gene and nowhere else"""
    Ge = len(cases.ENDS_ETA0)
    mo = oracle.model(cases.counts_small(Ge, cases.S), cases.X, cases.ENDS_EXPO, Ge, n_threads=4)
    gq = oracle.generated_quantities(mo, cases.ends_draws(700), 1.0, seed=1)
    assert (gq[:, 0] == 0).all()
    assert (gq[:, 1:4] == cases.SATURATED).all()
    bad = np.arange(700) % cases.ENDS_INVALID_EVERY == 0
    assert (gq[bad, 4] == cases.INVALID).all() and (gq[~bad, 4] < 10000).all()
    s = cases.summary_numpy(gq, 0.025, 0.975)
    assert (s[4, :, 3] == cases.INVALID).all() and (s[4, :, 2] < 100).all()      # the invalid draws sort last
