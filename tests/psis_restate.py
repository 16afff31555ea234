"""numpy restatement of the Pareto-k diagnostic (include/ppcx.h ppcx_fit_psis, ppcseq_amd/csrc/ppcx_psis.h): loo's
psis(r, r_eff = NA) tail fit written out on arrays from the published algorithm (Vehtari et al., JMLR 2024; Zhang and
Stephens 2009). Shared by tests/test_psis_host.py (CPU) and tests/test_gpu_psis.py (device)."""
import math

import numpy as np

PRIOR = 3.0
MIN_WEIGHT = 10 * np.finfo(np.float64).eps


def tail_len(N):
    return int(math.ceil(min(0.2 * N, 3.0 * math.sqrt(N))))


def gpdfit_k(x):
    """loo's gpdfit on the ascending x[0 .. M): the mean k of the profile fit, before the prior adjustment"""
    M = x.size
    m = 30 + int(math.floor(math.sqrt(M)))
    xstar = x[int(math.floor(M / 4 + 0.5)) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / PRIOR / xstar
        k = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
        ell = M * (np.log(-theta / k) - k - 1.0)
        mx = np.nan if np.isnan(ell).any() else ell.max()
        w = np.exp(ell - mx)
        w = w / w.sum()
        keep = ~(w < MIN_WEIGHT)
        w = w[keep] / w[keep].sum()
        th = float(np.sum(w * theta[keep]))
        return float(np.mean(np.log1p(-th * x)))


def khat(v):
    """k-hat of one column: NaN or +Inf anywhere -> NaN; -Inf entries left out; too short a tail or a constant one -> +Inf"""
    v = np.asarray(v, dtype=np.float64).ravel()
    if np.isnan(v).any() or (v == np.inf).any():
        return np.nan
    s = np.sort(v[v != -np.inf])
    N = s.size
    M = tail_len(N)
    if M < 5 or M >= N:
        return np.inf
    mx, c = s[-1], s[N - M - 1]
    tail = s[N - M:]
    if tail[0] == mx:
        return np.inf
    x = np.exp(tail - mx) - math.exp(c - mx)
    k = gpdfit_k(x)
    kh = (M * k + 5.0) / (M + 10.0)
    return np.inf if np.isnan(kh) else kh


def column_values(theta, r):
    """the values whose k-hat rstan's summary reports for a parameter: 1/2 log1p(theta^2) + r"""
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return 0.5 * np.log1p(theta * theta) + np.asarray(r, dtype=np.float64)


def log_ratios(log_p, log_g):
    """r = log_p - log_g, -Inf where either is not finite"""
    log_p, log_g = np.asarray(log_p, dtype=np.float64), np.asarray(log_g, dtype=np.float64)
    ok = np.isfinite(log_p) & np.isfinite(log_g)
    return np.where(ok, log_p - np.where(ok, log_g, 0.0), -np.inf)


def log_g(draws, mu, omega):
    """Stan's meanfield calc_log_g at each draw (row): -1/2 sum_d ((theta_d - mu_d) exp(-omega_d))^2"""
    z = (np.asarray(draws, dtype=np.float64) - mu[None, :]) * np.exp(-omega)[None, :]
    return -0.5 * np.sum(z * z, axis=1)


def gpd_sample(rng, k, n, sigma=1.0):
    """n draws of a generalised Pareto distribution with shape k > 0 (inverse cdf)"""
    u = rng.uniform(size=n)
    return sigma * (np.power(1.0 - u, -k) - 1.0) / k


def normal_ratios(rng, sigma2, n):
    """log ratios of a normal target N(0, sigma2) under a standard normal proposal: the importance weights have Pareto shape
    k = 1 - 1 / sigma2"""
    z = rng.normal(size=n)
    return -0.5 * z * z / sigma2 + 0.5 * z * z
