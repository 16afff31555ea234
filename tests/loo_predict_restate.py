"""numpy restatement of the leave-one-out predictive interval and LOO-PIT per cell (include/ppcx.h ppcx_fit_loo_predict,
ppcseq_amd/csrc/ppcx_loo_predict.h) on top of tests/loo_restate.py's psis_log_weights: what loo::E_loo(yrep, psis, type = "mean" /
"quantile") and bayesplot's ppc_loo_pit compute from a cell's log-likelihoods ll [n], its predictive counts x [n] and its
observed count y. Shared by tests/test_loo_predict_host.py (CPU) and tests/test_gpu_loo_predict.py (device)."""
import numpy as np

from tests import loo_restate as L

FIELDS = ("mean", "lower", "upper", "pit_lt", "pit_le", "khat")
INVALID = 2147483647


def weights(ll, r_eff=1.0):
    """(normalised weights [n] in draw order -- 0 for a draw whose ratio is -Inf --, k-hat). psis_log_weights sorts the
    participating draws with a stable sort: tied ratios take the tail's positions in draw order."""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    part = ll != np.inf
    lw, kh = L.psis_log_weights(-ll[part], r_eff)
    w = np.zeros(ll.size)
    w[part] = np.exp(lw - lw.max())
    return w / w.sum(), kh


def support(w, x, part):
    """distinct drawn values (ascending) of the participating draws and F at each"""
    vals = np.unique(x[part])
    return vals, np.array([np.sum(w[x <= v]) for v in vals])


def _star(F, p):
    """index of v*: the smallest drawn value with F >= p, else the largest"""
    hit = np.nonzero(F >= p)[0]
    return int(hit[0]) if hit.size else F.size - 1


def quantile(w, x, part, p):
    """(Q(p), v-, v*, condition number of the interpolation); v- = None where no drawn value is below v*"""
    vals, F = support(w, x, part)
    q = _star(F, p)
    if q == 0:
        return float(vals[0]), None, int(vals[0]), 0.0
    vm, vs = float(vals[q - 1]), float(vals[q])
    cond = (vs - vm) / (F[q] - F[q - 1])
    return vm + (vs - vm) * (p - F[q - 1]) / (F[q] - F[q - 1]), int(vm), int(vs), cond


def _fma(a, b, c):
    """a * b + c with one rounding"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def type7(x, p):
    """type-7 quantile in the form of the posterior-predictive kernels: h = (n - 1) p rounded, lo = floor(h), one fma"""
    import math
    xs = np.sort(np.asarray(x, dtype=np.int64))
    n = xs.size
    h = float(n - 1) * p
    lo = min(max(int(math.floor(h)), 0), n - 1)
    if lo >= n - 1:
        return float(xs[lo])
    v0, v1 = float(xs[lo]), float(xs[lo + 1])
    return _fma(h - lo, v1 - v0, v0)


def point(ll, x, y, r_eff=1.0, excluded=False, p_lo=0.025, p_hi=0.975):
    """dict of the six fields of one cell, plus `cond` (lower, upper): the interpolations' condition numbers, and `support`
    ((v-, v*) of lower and of upper)"""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    x = np.asarray(x, dtype=np.int64).ravel()
    n = ll.size
    nan = dict({k: np.nan for k in FIELDS}, cond=(0.0, 0.0), support=((None, None), (None, None)))
    r = -ll
    if np.isnan(r).any() or (not excluded and (r == np.inf).any()) or (x == INVALID).any():
        return nan
    if excluded:
        return dict(mean=float(x.sum()) / n, lower=type7(x, p_lo), upper=type7(x, p_hi), pit_lt=float(np.sum(x < y)) / n,
                    pit_le=float(np.sum(x <= y)) / n, khat=np.nan, cond=(0.0, 0.0), support=((None, None), (None, None)))
    part = ll != np.inf
    if not part.any():
        return nan
    w, kh = weights(ll, r_eff)
    lo, hi = quantile(w, x, part, p_lo), quantile(w, x, part, p_hi)
    return dict(mean=float(np.sum(w * x)), lower=lo[0], upper=hi[0], pit_lt=float(np.sum(w[x < y])),
                pit_le=float(np.sum(w[x <= y])), khat=kh, cond=(lo[3], hi[3]), support=(lo[1:3], hi[1:3]))


def borderline(ll, x, p, r_eff=1.0, eps=1e-9):
    """Whether Q(p) of a non-excluded cell sits where summation order may legitimately pick a neighbouring support point:
    |F(v) - p| <= eps for v in {v-, v*}, or F(v*) - F(v-) < eps."""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    x = np.asarray(x, dtype=np.int64).ravel()
    part = ll != np.inf
    w, _ = weights(ll, r_eff)
    vals, F = support(w, x, part)
    q = _star(F, p)
    if abs(F[q] - p) <= eps:
        return True
    return q > 0 and (abs(F[q - 1] - p) <= eps or F[q] - F[q - 1] < eps)


def check(got, ref, ll=None, x=None, r_eff=1.0, p_lo=0.025, p_hi=0.975, what=""):
    """The issue's tolerances for one cell: got [6] against point()'s dict. Returns the number of quantiles skipped as
    borderline (0, 1 or 2)."""
    skipped = 0
    for i, k in enumerate(FIELDS):
        g, r = float(got[i]), ref[k]
        if np.isnan(r) or not np.isfinite(r):
            assert (np.isnan(r) and np.isnan(g)) or g == r, (what, k, g, r)
            continue
        tol = 1e-12 * max(1.0, abs(r))
        if k in ("lower", "upper"):
            j = 0 if k == "lower" else 1
            if ll is not None and not np.isnan(ref["khat"]) and borderline(ll, x, (p_lo, p_hi)[j], r_eff):
                skipped += 1
                continue
            vm, vs = ref["support"][j]
            if vs is not None:                                   # the same support points: the value lies between them
                assert (vs if vm is None else vm) - tol <= g <= vs + tol, (what, k, g, vm, vs)
            tol += 1e-12 * ref["cond"][j]
        assert abs(g - r) <= tol, (what, k, g, r, abs(g - r), tol)
    return skipped
