"""numpy restatement of the fit summary's per-column statistics (include/ppcx.h ppcx_fit_summary, ppcseq_amd/csrc/ppcx_summary.h):
direct autocovariance, scipy rankdata / ndtri, the Geyer truncation written out on arrays as rstan's monitor() does. Shared by
tests/test_summary_host.py (CPU) and tests/test_gpu_summary.py (device)."""
import math

import numpy as np

FIELDS = ("mean", "sd", "q05", "q50", "q95", "rhat", "ess_bulk", "ess_tail")


def q7(s, p):
    """type-7 quantile of the sorted s, evaluated as the header does (s[lo] + (h - lo)(s[lo + 1] - s[lo]))"""
    N = s.size
    h = (N - 1) * p
    fl = math.floor(h)
    lo = int(fl)
    if lo >= N - 1:
        return float(s[N - 1])
    return float(s[lo] + (h - fl) * (s[lo + 1] - s[lo]))


def split(x):
    """x [M, n] -> [2M, n // 2]: chain c gives row 2c (its first n' draws) and 2c + 1 (its last n')"""
    M, n = x.shape
    nh = n // 2
    out = np.empty((2 * M, nh))
    out[0::2] = x[:, :nh]
    out[1::2] = x[:, n - nh:]
    return out


def ranks(v):
    from scipy.stats import rankdata
    return rankdata(v.ravel(), method="average").reshape(v.shape)


def rank_z(v):
    from scipy.special import ndtri
    return ndtri((ranks(v) - 0.375) / (v.size + 0.25))


def rhat_seq(z):
    nh = z.shape[1]
    B = nh * z.mean(axis=1).var(ddof=1)
    W = z.var(axis=1, ddof=1).mean()
    return math.sqrt((B / W + nh - 1) / nh)


def ess_seq(z):
    m, nh = z.shape
    c = z - z.mean(axis=1, keepdims=True)

    def acov(t):                                  # chain-averaged, direct; computed for the lags the truncation reaches
        return np.mean(np.sum(c[:, :nh - t] * c[:, t:], axis=1) / nh)

    mean_var = acov(0) * nh / (nh - 1)
    var_plus = mean_var * (nh - 1) / nh + z.mean(axis=1).var(ddof=1)
    if not var_plus > 0:
        return float("nan")

    class Rho:
        def __getitem__(self, t):
            return 1 - (mean_var - acov(t)) / var_plus
    rho = Rho()
    rh = np.zeros(nh + 2)
    rh[0], rh[1] = 1.0, rho[1]
    t, even, odd = 0, 1.0, rho[1]
    while t < nh - 5 and even + odd > 0:
        t += 2
        even, odd = rho[t], rho[t + 1]
        if even + odd >= 0:
            rh[t], rh[t + 1] = even, odd
    max_t = t
    if even > 0:
        rh[max_t] = even
    for t in range(2, max_t - 1, 2):
        if rh[t] + rh[t + 1] > rh[t - 2] + rh[t - 1]:
            rh[t] = rh[t + 1] = (rh[t - 2] + rh[t - 1]) / 2
    tau = -1 + 2 * np.sum(rh[:max_t]) + rh[max_t]
    tau = max(tau, 1 / math.log10(m * nh))
    return m * nh / tau


def summary_column(x):
    """x [M, n] -> dict of the eight fields (and `ranks` of the split values, chain-major sequence order)"""
    x = np.asarray(x, dtype=np.float64)
    M, n = x.shape
    out = dict.fromkeys(FIELDS, float("nan"))
    out["ranks"] = None
    if not np.all(np.isfinite(x)):
        return out
    flat = x.ravel()
    s = np.sort(flat)
    out.update(mean=flat.sum() / flat.size, sd=float(np.std(flat, ddof=1)) if flat.size > 1 else float("nan"),
               q05=q7(s, 0.05), q50=q7(s, 0.5), q95=q7(s, 0.95))
    nh = n // 2
    if nh < 2:
        return out
    sp = split(x)
    ss = np.sort(sp.ravel())
    if not ss[0] < ss[-1]:
        return out
    q05, med, q95 = q7(ss, 0.05), q7(ss, 0.5), q7(ss, 0.95)
    z = rank_z(sp)
    out["ranks"] = ranks(sp).ravel()
    rb, eb = rhat_seq(z), ess_seq(z)
    zf = rank_z(np.abs(sp - med))
    with np.errstate(invalid="ignore", divide="ignore"):
        rf = rhat_seq(zf)
    e05, e95 = ess_seq((sp <= q05).astype(float)), ess_seq((sp <= q95).astype(float))
    out.update(rhat=float(np.fmax(rb, rf)), ess_bulk=eb, ess_tail=float(np.fmin(e05, e95)))
    return out
