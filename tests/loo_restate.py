"""numpy restatement of PSIS-LOO per observed cell (include/ppcx.h ppcx_fit_loo / ppcx_fit_get_log_lik,
ppcseq_amd/csrc/ppcx_loo.h): the cell's log-likelihood over the draws, and loo's psis() / loo() pointwise columns written out
on arrays from the published algorithm (Vehtari, Gelman, Gabry 2017, "Practical Bayesian model evaluation using leave-one-out
cross-validation and WAIC"; Vehtari et al., JMLR 2024). The tail fit is tests/psis_restate.py's. Shared by
tests/test_loo_restate.py, tests/test_loo_host.py (CPU) and tests/test_gpu_loo.py (device)."""
import math

import numpy as np

from tests import psis_restate as P

FIELDS = ("elpd_loo", "p_loo", "looic", "khat")


def tail_len(N, r_eff=1.0):
    """M = ceil(min(0.2 N, 3 sqrt(N / r_eff)))"""
    return int(math.ceil(min(0.2 * N, 3.0 * math.sqrt(N / r_eff))))


def log_lik(y, eta, sigma_raw):
    """neg_binomial_2_log_lpmf(y | eta, phi = exp(-sigma_raw)) with every constant kept (scipy's nbinom.logpmf)"""
    from scipy import stats
    phi = np.exp(-np.asarray(sigma_raw, dtype=np.float64))
    mu = np.exp(np.asarray(eta, dtype=np.float64))
    return stats.nbinom.logpmf(y, phi, phi / (phi + mu))


def logsumexp(v):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return -np.inf
    mx = v.max()
    if mx == -np.inf:
        return -np.inf
    return float(mx + np.log(np.sum(np.exp(v - mx))))


def qgpd(p, k, sigma):
    return sigma * np.expm1(-k * np.log1p(-p)) / k


def psis_log_weights(r, r_eff=1.0):
    """loo's do_psis_i on the finite log ratios r: (unnormalised log weights in the frame shifted by max(r), k-hat). The tail
    (the M largest, by a stable sort) is replaced by log(qgpd((j - 1/2) / M; k-hat, sigma) + exp(cutoff)) where k-hat is finite
    and sigma > 0; every weight is truncated at the largest raw one (0 in this frame)."""
    r = np.asarray(r, dtype=np.float64)
    N = r.size
    lw = r - r.max()
    M = tail_len(N, r_eff)
    kh = np.inf
    if M >= 5 and M < N:
        ix = np.argsort(lw, kind="stable")
        s = lw[ix]
        tail = s[N - M:]
        if tail[0] != tail[-1]:
            cut = s[N - M - 1]
            x = np.exp(tail) - math.exp(cut)
            k = P.gpdfit_k(x)
            theta = _theta_hat(x)
            sigma = -k / theta
            kh = (M * k + 5.0) / (M + 10.0)
            kh = np.inf if np.isnan(kh) else kh
            if np.isfinite(kh) and sigma > 0:
                p = (np.arange(1, M + 1) - 0.5) / M
                with np.errstate(invalid="ignore", divide="ignore"):
                    lw[ix[N - M:]] = np.log(qgpd(p, kh, sigma) + math.exp(cut))
    return np.minimum(lw, 0.0), kh


def _theta_hat(x):
    """theta^ of loo's gpdfit (tests/psis_restate.py gpdfit_k composes the same steps)"""
    M = x.size
    m = 30 + int(math.floor(math.sqrt(M)))
    xstar = x[int(math.floor(M / 4 + 0.5)) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / P.PRIOR / xstar
        k = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
        ell = M * (np.log(-theta / k) - k - 1.0)
        mx = np.nan if np.isnan(ell).any() else ell.max()
        w = np.exp(ell - mx)
        w = w / w.sum()
        keep = ~(w < P.MIN_WEIGHT)
        w = w[keep] / w[keep].sum()
        return float(np.sum(w * theta[keep]))


def loo_point(ll, r_eff=1.0, excluded=False):
    """(elpd_loo, p_loo, looic, khat) of one cell from its log-likelihood over the draws. Log ratios r = -ll: a NaN or +Inf
    ratio (ll NaN or -Inf) makes the cell NaN; a -Inf ratio (ll = +Inf) takes no part. An excluded cell is already held out:
    elpd_loo = lpd, p_loo = 0, khat = NaN."""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    r = -ll
    if np.isnan(r).any() or (not excluded and (r == np.inf).any()):
        return (np.nan,) * 4
    ll = ll[r != -np.inf]
    N = ll.size
    lpd = logsumexp(ll) - math.log(N) if N else np.nan
    if excluded:
        return lpd, 0.0, -2.0 * lpd, np.nan
    lw, kh = psis_log_weights(-ll, r_eff)
    elpd = logsumexp(lw + ll) - logsumexp(lw)
    return elpd, lpd - elpd, -2.0 * elpd, kh


def loo_columns(ll, r_eff=None, excluded=None):
    """loo_point of every column of ll [n_draws, n_cells]: [n_cells, 4]"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.shape[1]
    r_eff = np.ones(n) if r_eff is None else np.asarray(r_eff, dtype=np.float64).ravel()
    excluded = np.zeros(n, bool) if excluded is None else np.asarray(excluded, bool).ravel()
    return np.array([loo_point(ll[:, i], r_eff[i], excluded[i]) for i in range(n)]).reshape(n, 4)


def estimates(pointwise, excluded=None):
    """loo's estimates for elpd_loo, p_loo and looic over the non-excluded cells: (sum, sqrt(n var)) with var of ddof 1"""
    out = {}
    for i, name in enumerate(FIELDS[:3]):
        v = np.asarray(pointwise[..., i], dtype=np.float64).ravel()
        if excluded is not None:
            v = v[~np.asarray(excluded, bool).ravel()]
        n = v.size
        se = math.sqrt(n * np.var(v, ddof=1)) if n > 1 else np.nan
        out[name] = (float(np.sum(v)), se)
    return out
