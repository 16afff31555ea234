"""Designed points of the predictive sampler (ppcseq_amd/csrc/ppcx_math.h nb2_log_rng) and the goodness-of-fit helper that holds
its integers to the negative binomial itself: a chi-square test against the exact pmf / cdf of scipy.stats.nbinom(phi,
phi / (phi + mu)). Shared by tests/test_nb_rng_distribution.py (the oracle and the CPU emulation) and tests/test_gpu_nb_rng.py (the
shipped kernels through Model.fit_from_draws and Fit.ppc), which build the same models and draws here, so that what the device
must return is known from the oracle before it runs.

Each point names the regime it is there for:"""
import math
from fractions import Fraction

import numpy as np
from scipy import stats

# (mu, phi)
POINTS = (
    (0.05, 0.5),      # Knuth, boost, nearly all zeros
    (3.0, 0.5),       # Knuth
    (8.0, 2.0),       # lambda = gamma mu / phi crosses 10 within the cell: both Poisson branches
    (10.0, 50.0),     # lambda near 10
    (12.0, 1.0),
    (50.0, 4.0),
    (1e3, 0.01),      # boost, tiny phi
    (200.0, 3.4e-4),  # tiny phi, the dispersion table's lower end
    (1e4, 1e4),
    (1e6, 50.0),
    (0.5, 1e6),       # Poisson limit
    (9.5, 1e5),       # below the Knuth / PTRS switch
    (10.5, 1e5),      # above it
    (3e8, 5.0),       # mass above 2^30: the saturated value is a bin of its own
    (2.0, 0.999),     # just below the boost switch
    (2.0, 1.0),       # at the boost switch
)
SEEDS = (1, 2, 3)                 # fixed in advance
P_MIN = 1e-4                      # a cap on the p-value of every (point, seed, path), not a measurement
N_CPU = 200000                    # draws per point of the CPU tests: what the weakest mutants need
SATURATED = 1073741823            # nb2_log_rng above 2^30
INVALID = 2147483647              # nb2_log_rng of an invalid draw: sorts last
MAX_BINS, MIN_EXPECTED = 40, 5.0

_bins = {}


def _edges(mu, phi):
    """Upper ends (inclusive) of up to MAX_BINS bins of equal probability and their cdf; the last bin runs to infinity. The cdf
    is censored at SATURATED (every larger count is that value), which is an edge of its own where it carries mass."""
    key = (float(mu), float(phi))
    if key not in _bins:
        d = stats.nbinom(phi, phi / (phi + mu))
        q = d.ppf(np.arange(1, MAX_BINS) / MAX_BINS)
        e = np.unique(np.minimum(q[np.isfinite(q)], SATURATED - 1).astype(np.int64))
        if d.sf(SATURATED - 1) > 0.0 and (e.size == 0 or e[-1] < SATURATED - 1):
            e = np.append(e, SATURATED - 1)
        _bins[key] = (e, d.cdf(e))
    return _bins[key]


def chi2_gof(x, mu, phi):
    """(chi-square statistic, degrees of freedom, p-value) of the integer draws x against NB(mean mu, size phi). Bins of equal
    probability, at most 40, merged from the sparse tail inwards until every expected count is >= 5."""
    x = np.minimum(np.asarray(x).ravel().astype(np.int64), SATURATED)
    n = x.size
    e, c = _edges(mu, phi)
    prob = np.diff(np.concatenate([[0.0], c, [1.0]]))
    obs = np.bincount(np.searchsorted(e, x, side="left"), minlength=e.size + 1).astype(np.float64)
    exp = n * prob
    obs, exp = list(obs), list(exp)
    i = len(exp) - 1
    while i > 0:                                  # the sparse tail first, then any sparse bin left of it
        if exp[i] < MIN_EXPECTED:
            exp[i - 1] += exp.pop(i); obs[i - 1] += obs.pop(i)
        i -= 1
    while len(exp) > 1 and exp[0] < MIN_EXPECTED:
        exp[1] += exp.pop(0); obs[1] += obs.pop(0)
    obs, exp = np.array(obs), np.array(exp)
    assert obs.size >= 2, "fewer than two bins: nothing to test"
    stat = float(np.sum((obs - exp) ** 2 / exp))
    df = int(obs.size - 1)
    return stat, df, float(stats.chi2.sf(stat, df))


# ---- the models and draws of the GPU tests ---------------------------------------------------------------------------------------
G = K = len(POINTS)
S = 5
N_WAVE = 4096                     # rows of the wavefront-per-cell path (no resampling)
N_ROWS = 64                       # rows that the two workgroup paths resample from
N_LDS, N_SCRATCH = 39680, 39681   # predictive draws per cell: the most that LDS holds, the first in the global scratch buffer
X = np.stack([np.ones(S), np.array([0.0, 1.0, 0.0, 1.0, 1.0])], axis=1)
# the variant: two exposures and the 0 / 1 column give three kinds of cell per gene: (e0, 0) cells 0, 2; (e1, 1) cells 1, 3; (e0, 1) cell 4
EXPO_VARIANT = np.array([0.25, -0.5, 0.25, -0.5, 0.25])
SLOPE_VARIANT = 0.375
CELL_KINDS = ((0, 2), (1, 3), (4,))


def offsets(G, C, K):
    """Positions in the unconstrained vector (oracle/ppc_oracle.c offsets)."""
    a1 = 3 + G
    sr = a1 + K + max(C - 2, 0) * K
    return {"intercept": 3, "alpha1": a1, "sigma_raw": sr, "D": sr + G + 3}


def counts_small(G, S):
    return (np.arange(G * S, dtype=np.int32).reshape(G, S) * 7) % 23


def designed_draws(n, variant=False):
    """[1, n, D], every row identical: intercept_g = ln mu_g, sigma_raw_g = -ln phi_g, the slopes SLOPE_VARIANT in the variant,
    everything else 0."""
    o = offsets(G, 2, K)
    u = np.zeros(o["D"])
    for g, (mu, phi) in enumerate(POINTS):
        u[o["intercept"] + g] = math.log(mu)
        u[o["sigma_raw"] + g] = -math.log(phi)
        if variant:
            u[o["alpha1"] + g] = SLOPE_VARIANT
    return np.tile(u, (1, n, 1))


def exposure(variant=False):
    return EXPO_VARIANT.copy() if variant else np.zeros(S)


def cell_mu(g, s, variant=False):
    """The cell's mean in fp64 from the same draws: exp(exposure_s + X_s . T_g)"""
    mu = POINTS[g][0]
    if not variant:
        return mu
    return math.exp(EXPO_VARIANT[s] + X[s, 0] * math.log(mu) + X[s, 1] * SLOPE_VARIANT)


def pooled_tests(rng, variant=False):
    """[(gene, cells, mu, phi, (stat, df, p))] of counts_rng [n, K, S]: the cells of a gene that share (mu, phi) pooled"""
    out = []
    for g in range(rng.shape[1]):
        for cells in (CELL_KINDS if variant else (tuple(range(S)),)):
            mu, phi = cell_mu(g, cells[0], variant), POINTS[g][1]
            out.append((g, cells, mu, phi, chi2_gof(rng[:, g, list(cells)], mu, phi)))
    return out


# ---- the summary in numpy, independent of oracle.summarise -----------------------------------------------------------------------
def _fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic; a Fraction converts to the nearest double)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def quantile7(sorted_col, p):
    """R's type-7 quantile of a sorted integer column as the kernels form it: fma(h - floor h, v1 - v0, v0), h = (n - 1) p"""
    n = sorted_col.size
    h = float(n - 1) * float(p)
    lo = int(math.floor(h))
    if lo >= n - 1:
        return float(sorted_col[n - 1])
    v0, v1 = float(sorted_col[lo]), float(sorted_col[lo + 1])
    return _fma(h - lo, v1 - v0, v0)


def summary_numpy(rng, p_lo, p_hi):
    """[K, S, 4] mean, sample sd, the two quantiles of counts_rng [n, K, S]"""
    n, K_, S_ = rng.shape
    out = np.zeros((K_, S_, 4))
    x = rng.astype(np.float64)
    out[..., 0] = x.mean(0)
    out[..., 1] = x.std(0, ddof=1) if n > 1 else np.nan
    srt = np.sort(rng, axis=0)
    for g in range(K_):
        for s in range(S_):
            out[g, s, 2] = quantile7(srt[:, g, s], p_lo)
            out[g, s, 3] = quantile7(srt[:, g, s], p_hi)
    return out


def assert_summary(ci, rng, p_lo, p_hi, what):
    ref = summary_numpy(rng, p_lo, p_hi)
    assert np.array_equal(ref[..., 2:], ci[..., 2:]), (what, "quantiles", np.argwhere(ref[..., 2:] != ci[..., 2:])[:4].tolist())
    if rng.shape[0] == 1:
        assert np.isnan(ci[..., 1]).all(), (what, "sd of one draw")
        assert np.array_equal(ref[..., 0], ci[..., 0]), (what, "mean of one draw")
        return
    err = np.abs(ref[..., :2] - ci[..., :2])
    tol = 1e-11 * np.abs(ref[..., :2])
    assert np.all(err <= tol), (what, "mean / sd", float(np.max(err / np.maximum(tol, 1e-300))))


# ---- the ends of the range -------------------------------------------------------------------------------------------------------
# genes of the model of the ends: eta of cell 0 (exposure 0.5) and phi; the last gene is valid with sigma_raw = 800 (phi = 0:
# an invalid draw) in every seventh row
ENDS_EXPO = np.array([0.5, -0.25, 0.0, 0.25, -0.5])
ENDS_ETA0 = (-750.0, 699.5, 705.0, 710.0, math.log(50.0) + 0.5)
ENDS_PHI = (1.0, 1.0, 1.0, 1.0, 4.0)
ENDS_INVALID_EVERY = 7


def ends_draws(n):
    """[1, n, D] for the model of the ends (G = K = 5, S = 5, the design X)"""
    Ge = len(ENDS_ETA0)
    o = offsets(Ge, 2, Ge)
    u = np.zeros((n, o["D"]))
    for g in range(Ge):
        u[:, o["intercept"] + g] = ENDS_ETA0[g] - ENDS_EXPO[0]
        u[:, o["sigma_raw"] + g] = -math.log(ENDS_PHI[g])
    u[::ENDS_INVALID_EVERY, o["sigma_raw"] + Ge - 1] = 800.0
    return u[None]
