"""An independent restatement of the exact leave-one-out predictive tails and interval per cell
(ppcseq_amd/csrc/ppcx_loo_exact.h) with scipy.stats.nbinom and numpy, and the CPU build of the header (tests/loo_exact_host).
The weights are tests/loo_predict_restate.weights (a NUTS fit) and tests/loo_ap_restate.weights (an ADVI fit: its ratio rule),
imported, not copied; the weighted cdf is the weighted sum of scipy's cdfs, the quantile the first integer of a numpy search; a
cell that a NUTS fit excludes is tests/ppc_exact_restate.point itself (the plain average). Nothing here is shared with the
code under test. Shared by tests/test_loo_exact_host.py (CPU) and tests/test_gpu_loo_exact.py (device).

WEIGHTED_MEASURED: the largest error of the CPU build against this restatement in khat, mean and sd over
tests/loo_exact_cases.designed(), in units of max(1, |ref|). It stays below the 1e-12 of loo_predict_restate.check's rule for
weighted sums, so that rule is the bound (WEIGHTED_BOUND) and no 4 x allowance is taken."""
import ctypes as C

import numpy as np

from tests import host_build
from tests import loo_ap_restate as AP
from tests import loo_predict_restate as LP
from tests import ppc_exact_restate as E

FIELDS = E.FIELDS + ("khat",)                 # kLooExactFields, in order
P2, TC = E.P2, E.TC
TAILS_BOUND, TAILS_ABS = E.TAILS_BOUND, E.TAILS_ABS
WEIGHTED_MEASURED = 6.0e-15                   # tests/test_loo_exact_host.py::test_header_matches_restatement prints it
WEIGHTED_BOUND = 1e-12


def host_lib():
    dp = C.POINTER(C.c_double)
    return host_build.host_lib("loo_exact", {
        "loo_exact_host_cell": ([dp, dp, dp, dp, C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, dp], C.c_int),
        "loo_exact_host_ppc_cell": ([dp, dp, C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp], None),
        "loo_exact_host_log_pmf": ([dp, dp, C.c_long, C.c_int, dp], None)})


def _col(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host_cell(h, ll, eta, sigma_raw, y, log_ratio=None, excluded=False, r_eff=1.0, tc=1.0, p_lo=0.025, p_hi=0.975):
    """(the cell's fields [10], the largest step count) of the CPU build"""
    ll, eta, sg = _col(ll), _col(eta), _col(sigma_raw)
    lr = None if log_ratio is None else _col(log_ratio)
    out = np.zeros(len(FIELDS))
    it = h.loo_exact_host_cell(_dp(ll), _dp(eta), _dp(sg), _dp(lr) if lr is not None else None, ll.size, int(y), int(excluded),
                               float(r_eff), float(tc), float(p_lo), float(p_hi), _dp(out))
    return out, it


def host_ppc_cell(h, eta, sigma_raw, y, excluded=False, tc=1.0, p_lo=0.025, p_hi=0.975):
    """ppc_exact_cell_host's fields [9] from the same CPU build"""
    eta, sg = _col(eta), _col(sigma_raw)
    out = np.zeros(len(E.FIELDS))
    h.loo_exact_host_ppc_cell(_dp(eta), _dp(sg), eta.size, int(y), int(excluded), float(tc), float(p_lo), float(p_hi), _dp(out))
    return out


def host_log_pmf(h, eta, sigma_raw, y):
    """the cell's own log-likelihood at every draw as a fit forms it (loo_ll: phi = exp(-sigma_raw))"""
    eta, sg = _col(eta), _col(sigma_raw)
    out = np.zeros(eta.size)
    h.loo_exact_host_log_pmf(_dp(eta), _dp(sg), eta.size, int(y), _dp(out))
    return out


# ---- the statistic

def weighted_cdf(k, eta, phi, w):
    """tests/ppc_exact_restate.mixture_cdf with weights in place of the plain average"""
    from scipy.stats import nbinom
    return float(np.sum(w * nbinom.cdf(k, phi, phi / (phi + np.exp(eta)))))


def quantile(p, eta, phi, w):
    """tests/ppc_exact_restate.quantile on the weighted cdf: the smallest integer k >= 0 with F(k) >= p"""
    if weighted_cdf(0, eta, phi, w) >= p:
        return 0
    lo, hi = 0, 1
    while weighted_cdf(hi, eta, phi, w) < p:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if weighted_cdf(mid, eta, phi, w) >= p:
            hi = mid
        else:
            lo = mid
    return hi


def cell_weights(ll, log_ratio=None, excluded=False, r_eff=1.0):
    """(normalised weights [n] in draw order, k-hat) of a weighted cell, "uniform" for the cell a NUTS fit excludes, None where
    the ratios make the cell NaN"""
    ll = _col(ll)
    if log_ratio is not None:
        w = AP.weights(ll, log_ratio, excluded)
        return None if w is None else (w[0], w[2])
    r = -ll
    if np.isnan(r).any() or (not excluded and (r == np.inf).any()):
        return None
    if excluded:
        return "uniform"
    if not (ll != np.inf).any():
        return None
    return LP.weights(ll, r_eff)


def point(ll, eta, sigma_raw, y, log_ratio=None, excluded=False, r_eff=1.0, tc=1.0, p_lo=0.025, p_hi=0.975):
    """dict of the ten fields of one cell, plus what check() needs for the allowance (eta, phi, w, p_lo, p_hi)"""
    from scipy.stats import nbinom
    eta = _col(eta)
    nan = {k: np.nan for k in FIELDS}
    nan.update(y=int(y), excluded=bool(excluded))
    w = cell_weights(ll, log_ratio, excluded, r_eff)
    if w is None:
        return nan
    if isinstance(w, str):                        # already held out: the posterior-predictive cell
        ref = E.point(eta, sigma_raw, y, excluded=excluded, tc=tc, p_lo=p_lo, p_hi=p_hi)
        ref["khat"] = np.nan
        if not np.isnan(ref["mean"]):
            ref["w"] = np.full(eta.size, 1.0 / eta.size)
        return ref
    w, kh = w
    phi = np.exp(-_col(sigma_raw)) * tc
    mu = np.exp(eta)
    if not (np.all(np.isfinite(eta)) and np.all(np.isfinite(phi)) and np.all(phi > 0) and np.all(np.isfinite(mu))):
        return nan
    p = phi / (phi + mu)
    mean = float(np.sum(w * mu))
    lower, upper = quantile(p_lo, eta, phi, w), quantile(p_hi, eta, phi, w)
    return dict(mean=mean, sd=float(np.sqrt(np.sum(w * (mu + mu * mu / phi)) + np.sum(w * (mu - mean) ** 2))),
                p_le=float(np.sum(w * nbinom.cdf(y, phi, p))), p_ge=float(np.sum(w * nbinom.sf(y - 1, phi, p))),
                lower=lower, upper=upper, y=int(y), excluded=bool(excluded), outside=bool(y < lower or y > upper), khat=kh,
                eta=eta, phi=phi, w=w, p_lo=p_lo, p_hi=p_hi)


def weighted_errors(got, ref):
    """the errors of khat, mean and sd in units of max(1, |ref|) (a k-hat that is not finite must be equal: error 0 or Inf)"""
    errs = []
    for i, k in ((0, "mean"), (1, "sd"), (9, "khat")):
        g, r = float(got[i]), float(ref[k])
        if not np.isfinite(r):
            errs.append(0.0 if (np.isnan(r) and np.isnan(g)) or g == r else np.inf)
        else:
            errs.append(abs(g - r) / max(1.0, abs(r)))
    return errs


def check(got, ref, what=""):
    """got [10] against point(): khat, mean, sd at WEIGHTED_BOUND max(1, |ref|); the tails at TAILS_BOUND (relative in the smaller,
    absolute in the larger); the interval ends equal, or one count apart where the restatement's own F at the count between them
    is within TAILS_BOUND of p (relative to min(p, 1 - p)): ppc_exact_restate.check's rules. Returns the number of ends that used
    the allowance."""
    if np.isnan(ref["mean"]):
        assert all(np.isnan(got[i]) for i in (0, 1, 2, 3, 4, 5, 8, 9)), (what, got)
        assert got[6] == ref["y"] and got[7] == ref["excluded"], (what, got)
        return 0
    errs = weighted_errors(got, ref)
    assert max(errs) <= WEIGHTED_BOUND, (what, errs, got, ref["mean"], ref["sd"], ref["khat"])
    err, ab = E.tails_errors(np.array([got[2]]), np.array([got[3]]), np.array([ref["p_le"]]), np.array([ref["p_ge"]]))
    assert err[0] <= TAILS_BOUND and ab[0] <= TAILS_ABS, (what, got[2], got[3], ref["p_le"], ref["p_ge"])
    used = 0
    for i, k, p in ((4, "lower", ref["p_lo"]), (5, "upper", ref["p_hi"])):
        if got[i] == ref[k]:
            continue
        assert abs(got[i] - ref[k]) == 1, (what, k, got[i], ref[k])
        f = weighted_cdf(int(min(got[i], ref[k])), ref["eta"], ref["phi"], ref["w"])
        assert abs(f - p) <= TAILS_BOUND * min(p, 1 - p), (what, k, got[i], ref[k], f, p)
        used += 1
    assert got[6] == ref["y"] and got[7] == ref["excluded"], (what, got)
    if not used:
        assert got[8] == ref["outside"], (what, got)
    return used
