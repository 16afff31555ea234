"""numpy restatement of the Monte-Carlo standard error of elpd_loo and the PSIS effective sample size per observed cell
(include/ppcx.h ppcx_fit_loo_mcse, ppcseq_amd/csrc/ppcx_loo.h steps 5 - 8): loo's `mcse_elpd_loo` in its deterministic form on
1 000 Blom scores and `psis_n_eff`, written out on arrays from the published package (Vehtari, Gelman, Gabry 2017; loo's
.mcse_elpd and psis_n_eff). The weights are tests/loo_restate.py's, the normal quantile scipy's. Shared by
tests/test_loo_mcse_host.py (CPU) and tests/test_gpu_loo_mcse.py (device)."""
import math

import numpy as np
from scipy.special import ndtri

from tests import loo_restate as L

FIELDS = L.FIELDS + ("mcse_elpd_loo", "n_eff")
N_SCORES = 1000


def blom_scores(n=N_SCORES):
    """Phi^-1((j - 3/8) / (n + 1/4)), j = 1 .. n: loo's zn"""
    return ndtri((np.arange(1, n + 1) - 0.375) / (n + 0.25))


def weights(ll, r_eff=1.0, excluded=False):
    """The normalised weights behind elpd_loo over the participating draws ll (no +Inf among them): PSIS weights of r = -ll
    (raw where k-hat is +Inf), uniform for an excluded cell"""
    if excluded:
        return np.full(ll.size, 1.0 / ll.size)
    lw, _ = L.psis_log_weights(-ll, r_eff)
    return np.exp(lw - L.logsumexp(lw))


def mcse_from_c(c, r_eff=1.0):
    """steps 7 - 8: sqrt(var(log1p(c z_j) over the j with 1 + c z_j > 0, ddof 1) / r_eff)"""
    t = c * blom_scores()
    x = np.log1p(t[1.0 + t > 0.0])
    return math.sqrt(np.var(x, ddof=1) / r_eff)


def mcse_point(ll, r_eff=1.0, excluded=False):
    """(elpd_loo, p_loo, looic, khat, mcse_elpd_loo, n_eff) of one cell from its log-likelihood over the draws"""
    base = L.loo_point(ll, r_eff, excluded)
    ll = np.asarray(ll, dtype=np.float64).ravel()
    if np.isnan(ll).any() or (not excluded and (ll == -np.inf).any()):
        return tuple(base) + (np.nan, np.nan)
    ll = ll[ll != np.inf]
    if ll.size == 0:
        return tuple(base) + (np.nan, np.nan)
    w = weights(ll, r_eff, excluded)
    n_eff = ll.size * r_eff if excluded else r_eff / np.sum(w * w)
    e = min(max(base[0], ll.min()), ll.max())          # elpd_loo lies there but for rounding: a constant column gives c = 0
    with np.errstate(invalid="ignore"):
        c = math.sqrt(np.sum((w * np.expm1(ll - e)) ** 2))
    return tuple(base) + (mcse_from_c(c, r_eff), n_eff)


def mcse_columns(ll, r_eff=None, excluded=None):
    """mcse_point of every column of ll [n_draws, n_cells]: [n_cells, 6]"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.shape[1]
    r_eff = np.ones(n) if r_eff is None else np.asarray(r_eff, dtype=np.float64).ravel()
    excluded = np.zeros(n, bool) if excluded is None else np.asarray(excluded, bool).ravel()
    return np.array([mcse_point(ll[:, i], r_eff[i], excluded[i]) for i in range(n)]).reshape(n, 6)


def mcse_loo_frame(ll, r_eff=1.0):
    """loo's .mcse_elpd as written, on exp(ll) itself (a non-excluded column without +-Inf that does not underflow):
    z = E + sd zn with E = exp(elpd_loo), sd = sqrt(sum w^2 (exp(ll) - E)^2); sqrt(var(log z[z > 0]) / r_eff)"""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    w = weights(ll, r_eff)
    E = math.exp(L.loo_point(ll, r_eff)[0])
    sd = math.sqrt(np.sum(w * w * (np.exp(ll) - E) ** 2))
    z = E + sd * blom_scores()
    return math.sqrt(np.var(np.log(z[z > 0]), ddof=1) / r_eff)
