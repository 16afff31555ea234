"""numpy restatement of PSIS-LOO per observed cell of an ADVI fit (include/ppcx.h ppcx_fit_loo_approx /
ppcx_fit_loo_predict_approx, ppcseq_amd/csrc/ppcx_loo_ap.h): loo::loo_approximate_posterior(log_lik, log_p, log_g) written out on
arrays from the published algorithm (Magnusson, Andersen, Jonasson, Vehtari 2019, "Bayesian leave-one-out cross-validation for
large data"). The smoothing is tests/loo_restate.py's psis_log_weights (its argsort is stable: tied ratios take the tail's
positions in draw order), the tail fit tests/psis_restate.py's, the predictive fields tests/loo_predict_restate.py's. Shared by
tests/test_loo_ap_host.py (CPU) and tests/test_gpu_loo_ap.py (device)."""
import math

import numpy as np

from tests import loo_predict_restate as R
from tests import loo_restate as L
from tests import psis_restate as P

FIELDS = L.FIELDS


def ratios(ll, a, excluded=False):
    """r = a - ll (an excluded cell: a alone), or None where the cell is NaN: a NaN in a or ll, a ratio of +Inf, an excluded
    cell with ll = +Inf"""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    a = np.asarray(a, dtype=np.float64).ravel()
    if np.isnan(a).any() or np.isnan(ll).any():
        return None
    with np.errstate(invalid="ignore"):
        r = a.copy() if excluded else a - ll
    if np.isnan(r).any() or (r == np.inf).any() or (excluded and (ll == np.inf).any()):
        return None
    return r


def log_weights(ll, a, excluded=False):
    """(log weights [n] in draw order, -Inf for a draw that takes no part; the participating mask; k-hat), or None where the
    cell is NaN (also: no participating draw)"""
    r = ratios(ll, a, excluded)
    if r is None:
        return None
    part = r != -np.inf
    if not part.any():
        return None
    lw = np.full(r.size, -np.inf)
    lw[part], kh = L.psis_log_weights(r[part], 1.0)
    return lw, part, kh


def loo_point(ll, a, excluded=False):
    """(elpd_loo, p_loo, looic, khat) of one cell from its log-likelihood and the fit's log ratios a = log_p - log_g"""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    w = log_weights(ll, a, excluded)
    if w is None:
        return (np.nan,) * 4
    lw, part, kh = w
    elpd = L.logsumexp(lw[part] + ll[part]) - L.logsumexp(lw[part])
    lpd = L.logsumexp(ll[part]) - math.log(part.sum())
    return elpd, 0.0 if excluded else lpd - elpd, -2.0 * elpd, kh


def loo_columns(ll, a, excluded=None):
    """loo_point of every column of ll [n_draws, n_cells]: [n_cells, 4]"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.shape[1]
    excluded = np.zeros(n, bool) if excluded is None else np.asarray(excluded, bool).ravel()
    return np.array([loo_point(ll[:, i], a, excluded[i]) for i in range(n)]).reshape(n, 4)


def weights(ll, a, excluded=False):
    """(normalised weights [n] in draw order, the participating mask, k-hat) or None"""
    w = log_weights(ll, a, excluded)
    if w is None:
        return None
    lw, part, kh = w
    e = np.exp(lw - lw[part].max())
    return e / e.sum(), part, kh


def predict_point(ll, a, x, y, excluded=False, p_lo=0.025, p_hi=0.975):
    """tests/loo_predict_restate.point's dict under these weights; an excluded cell is weighted like any other"""
    x = np.asarray(x, dtype=np.int64).ravel()
    nan = dict({k: np.nan for k in R.FIELDS}, cond=(0.0, 0.0), support=((None, None), (None, None)))
    w = weights(ll, a, excluded)
    if w is None or (x == R.INVALID).any():
        return nan
    w, part, kh = w
    lo, hi = R.quantile(w, x, part, p_lo), R.quantile(w, x, part, p_hi)
    return dict(mean=float(np.sum(w * x)), lower=lo[0], upper=hi[0], pit_lt=float(np.sum(w[x < y])),
                pit_le=float(np.sum(w[x <= y])), khat=kh, cond=(lo[3], hi[3]), support=(lo[1:3], hi[1:3]))


def borderline(ll, a, x, p, excluded=False, eps=1e-9):
    """tests/loo_predict_restate.borderline under these weights"""
    x = np.asarray(x, dtype=np.int64).ravel()
    w, part, _ = weights(ll, a, excluded)
    vals, F = R.support(w, x, part)
    q = R._star(F, p)
    if abs(F[q] - p) <= eps:
        return True
    return q > 0 and (abs(F[q - 1] - p) <= eps or F[q] - F[q - 1] < eps)


def predict_check(got, ref, ll, a, x, excluded=False, p_lo=0.025, p_hi=0.975, what=""):
    """tests/loo_predict_restate.check's tolerances for one cell, with the borderline cells judged under these weights: a
    quantile that `borderline` marks is taken out of the restatement's dict first. Returns how many were (0, 1 or 2)."""
    ref = dict(ref)
    got = list(got)
    skipped = 0
    if not np.isnan(ref["khat"]):
        for j, (k, p) in enumerate((("lower", p_lo), ("upper", p_hi))):
            if borderline(ll, a, x, p, excluded):
                skipped += 1
                ref[k] = got[1 + j] = np.nan                    # R.check compares NaN with NaN: nothing left to judge
    assert R.check(got, ref, None, x, 1.0, p_lo, p_hi, what) == 0
    return skipped
