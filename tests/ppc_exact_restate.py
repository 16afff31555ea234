"""An independent restatement of the exact posterior-predictive tails and interval per cell (ppcseq_amd/csrc/ppcx_ppc_exact.h)
with scipy.stats.nbinom and numpy, the references of the negative-binomial tails (ppcx_nbcdf.h), the CPU build of the two
headers (tests/ppc_exact_host) and the designed columns that the CPU and the device tests share. Nothing here is shared with
the code under test: the mixture cdf is the mean of scipy's cdfs, the quantile the first integer of a numpy search."""
import ctypes as C

import numpy as np

from tests import host_build

FIELDS = ("mean", "sd", "p_le", "p_ge", "lower", "upper", "y", "excluded", "outside")     # kPpcExactFields, in order
P2 = 2.4e-4                                   # a pass-2 tail probability (the README case: 0.05 / 21 / 10 rounded)
TC = 0.7352941                                # a pass-2 truncation compensation
# The bound of the negative-binomial tails: 4 x the largest error of the CPU build against the
# references over tails_points(), relative in the smaller tail where it exceeds 1e-300, absolute in the larger. The largest
# error measured is 3.8e-10 (at y = 2 580 228, phi = 1e-3, against scipy; 1.4e-11 against mpmath at y <= 2 001); the largest
# absolute error of either tail 4.8e-11; at most 360 steps of the continued fraction.
TAILS_MEASURED = 3.8e-10
TAILS_BOUND = 4 * TAILS_MEASURED
TAILS_ABS = 1e-8                              # a condition, not a measurement: either tail's absolute error


def host_lib():
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    return host_build.host_lib("ppc_exact", {
        "ppc_exact_host_tails": ([C.c_int, ip, dp, dp, dp, dp, ip], None),
        "ppc_exact_host_cell": ([dp, dp, C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp], C.c_int),
        "ppc_exact_host_rng": ([C.c_int, dp, dp, C.c_uint32, C.c_uint32, ip], None)})


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def host_tails(h, y, eta, phi):
    """(p_le, p_ge, steps of the continued fraction) of the CPU build at every point"""
    y = np.ascontiguousarray(y, dtype=np.int32)
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    le, ge, it = np.zeros(y.size), np.zeros(y.size), np.zeros(y.size, np.int32)
    h.ppc_exact_host_tails(y.size, _ip(y), _dp(eta), _dp(phi), _dp(le), _dp(ge), _ip(it))
    return le, ge, it


def host_cell(h, eta, sigma_raw, y, excluded=False, tc=1.0, p_lo=0.025, p_hi=0.975):
    """(the cell's fields [9], the largest step count) of the CPU build"""
    eta = np.ascontiguousarray(eta, dtype=np.float64).ravel()
    sg = np.ascontiguousarray(sigma_raw, dtype=np.float64).ravel()
    out = np.zeros(len(FIELDS))
    it = h.ppc_exact_host_cell(_dp(eta), _dp(sg), eta.size, int(y), int(excluded), float(tc), float(p_lo), float(p_hi), _dp(out))
    return out, it


def host_rng(h, eta, phi, k0, cell):
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    out = np.zeros(eta.size, np.int32)
    h.ppc_exact_host_rng(eta.size, _dp(eta), _dp(phi), int(k0), int(cell), _ip(out))
    return out


# ---- the negative-binomial tails

TAILS_Y = (0, 1, 2, 667, 2001, 10 ** 5, 2580228)
TAILS_PHI = (1e-3, 0.5, 5.0, 100.0, 1e5)
TAILS_MU = (0.01, 5.0, 667.0, 1e5, 2.6e6)
MP_MAX_Y = 5000


def tails_points():
    """(y, mu, phi) of the edge points: the grid, and for every (y, phi) the mean at which the continued fraction changes sides
    (x = (a + 1) / (a + b + 2) with a = phi, b = y + 1: mu = phi (y + 2) / (phi + 1)), just below and just above it."""
    pts = []
    for y in TAILS_Y:
        for phi in TAILS_PHI:
            sw = phi * (y + 2.0) / (phi + 1.0)
            for mu in TAILS_MU + (sw * 0.999, sw, sw * 1.001):
                pts.append((y, mu, phi))
    y, mu, phi = (np.array(v) for v in zip(*pts))
    return y.astype(np.int64), mu.astype(np.float64), phi.astype(np.float64)


def tails_reference(y, mu, phi):
    """(p_le, p_ge, both as floats, and as (value, smaller-tail-is-resolved) pairs): mpmath by direct summation of the pmf for
    y <= MP_MAX_Y -- at a working precision of 360 digits, so that a tail above 1e-300 formed as 1 - (the sum) keeps more than
    40 -- and scipy.stats.nbinom beyond. mu and phi are the doubles handed to the code under test (eta = log(mu) is rounded
    again: the reference is evaluated at exp(eta) as mpmath sees that double)."""
    import mpmath as mp
    from scipy.stats import nbinom
    le, ge = np.zeros(y.size), np.zeros(y.size)
    eta = np.log(mu)
    with mp.workdps(360):
        for i in range(y.size):
            yi = int(y[i])
            if yi > MP_MAX_Y:
                p = phi[i] / (phi[i] + np.exp(eta[i]))
                le[i], ge[i] = nbinom.cdf(yi, phi[i], p), nbinom.sf(yi - 1, phi[i], p)
                continue
            ph, m = mp.mpf(float(phi[i])), mp.exp(mp.mpf(float(eta[i])))
            x = ph / (ph + m)
            q = m / (ph + m)
            pm = mp.exp(ph * mp.log(x))                           # pmf(0)
            s, below = mp.mpf(0), mp.mpf(0)
            for k in range(yi + 1):
                if k == yi:
                    below = s
                s += pm
                pm = pm * (k + ph) / (k + 1) * q
            le[i], ge[i] = float(s), float(1 - below)
    return eta, le, ge


def tails_errors(got_le, got_ge, ref_le, ref_ge):
    """per point the error as the bound takes it (relative in the smaller tail where it exceeds 1e-300, absolute in the larger)
    and the largest absolute error of the two"""
    err = np.zeros(ref_le.size)
    ab = np.maximum(np.abs(got_le - ref_le), np.abs(got_ge - ref_ge))
    for i in range(ref_le.size):
        pairs = sorted(((ref_le[i], got_le[i]), (ref_ge[i], got_ge[i])))
        (rs, gs), (rl, gl) = pairs
        e = abs(gl - rl)
        e = max(e, abs(gs - rs) / rs if rs > 1e-300 else abs(gs - rs))
        err[i] = e
    return err, ab


# ---- the statistic

def mixture_cdf(k, eta, phi):
    from scipy.stats import nbinom
    p = phi / (phi + np.exp(eta))
    return float(np.mean(nbinom.cdf(k, phi, p)))


def quantile(p, eta, phi):
    """the smallest integer k >= 0 with the mixture cdf >= p: doubling from 1, then bisection"""
    if mixture_cdf(0, eta, phi) >= p:
        return 0
    lo, hi = 0, 1
    while mixture_cdf(hi, eta, phi) < p:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mixture_cdf(mid, eta, phi) >= p:
            hi = mid
        else:
            lo = mid
    return hi


def point(eta, sigma_raw, y, excluded=False, tc=1.0, p_lo=0.025, p_hi=0.975):
    from scipy.stats import nbinom
    eta = np.asarray(eta, dtype=np.float64).ravel()
    phi = np.exp(-np.asarray(sigma_raw, dtype=np.float64).ravel()) * tc
    mu = np.exp(eta)
    if not (np.all(np.isfinite(eta)) and np.all(np.isfinite(phi)) and np.all(phi > 0) and np.all(np.isfinite(mu))):
        r = {k: np.nan for k in FIELDS}
        r.update(y=int(y), excluded=bool(excluded))
        return r
    p = phi / (phi + mu)
    lower, upper = quantile(p_lo, eta, phi), quantile(p_hi, eta, phi)
    return dict(mean=float(np.mean(mu)), sd=float(np.sqrt(np.mean(mu + mu * mu / phi) + np.var(mu))),
                p_le=float(np.mean(nbinom.cdf(y, phi, p))), p_ge=float(np.mean(nbinom.sf(y - 1, phi, p))),
                lower=lower, upper=upper, y=int(y), excluded=bool(excluded), outside=bool(y < lower or y > upper),
                eta=eta, phi=phi, p_lo=p_lo, p_hi=p_hi)


def check(got, ref, what=""):
    """got [9] against point(): mean, sd 1e-12 relative; the tails at TAILS_BOUND (relative in the smaller, absolute in the
    larger); the interval ends equal, or one count apart where the restatement's own F at the count between them is within
    TAILS_BOUND of p (relative to min(p, 1 - p)). Returns the number of ends that used the allowance."""
    if np.isnan(ref["mean"]):
        assert all(np.isnan(got[i]) for i in (0, 1, 2, 3, 4, 5, 8)), (what, got)
        assert got[6] == ref["y"] and got[7] == ref["excluded"], (what, got)
        return 0
    for i, k in ((0, "mean"), (1, "sd")):
        assert abs(got[i] - ref[k]) <= 1e-12 * abs(ref[k]), (what, k, got[i], ref[k])
    err, ab = tails_errors(np.array([got[2]]), np.array([got[3]]), np.array([ref["p_le"]]), np.array([ref["p_ge"]]))
    assert err[0] <= TAILS_BOUND and ab[0] <= TAILS_ABS, (what, got[2], got[3], ref["p_le"], ref["p_ge"])
    used = 0
    for i, k, p in ((4, "lower", ref["p_lo"]), (5, "upper", ref["p_hi"])):
        if got[i] == ref[k]:
            continue
        assert abs(got[i] - ref[k]) == 1, (what, k, got[i], ref[k])
        f = mixture_cdf(int(min(got[i], ref[k])), ref["eta"], ref["phi"])
        assert abs(f - p) <= TAILS_BOUND * min(p, 1 - p), (what, k, got[i], ref[k], f, p)
        used += 1
    assert got[6] == ref["y"] and got[7] == ref["excluded"], (what, got)
    if not used:
        assert got[8] == ref["outside"], (what, got)
    return used


def designed():
    """designed columns: name, eta [n], sigma_raw [n], y, excluded, tc, p_lo, p_hi"""
    rng = np.random.default_rng(20)
    cs = []

    def add(name, eta, sg, y, excluded=False, tc=1.0, p=0.025):
        cs.append(dict(name=name, eta=np.asarray(eta, np.float64), sg=np.asarray(sg, np.float64), y=int(y), excluded=excluded, tc=tc,
                       p_lo=p, p_hi=1 - p))
    for n in (1, 20, 1000, 4000):
        add(f"constant draws n={n}", np.full(n, 4.2), np.full(n, -1.3), 60)
        add(f"constant draws pass 2 n={n}", np.full(n, 6.5), np.full(n, -2.0), 900, tc=TC, p=P2)
        add(f"wide eta n={n}", rng.normal(5.0, 1.5, n), rng.normal(-1.0, 0.1, n), 150, p=P2)
        add(f"phi spread n={n}", rng.normal(3.0, 0.1, n), rng.normal(0.0, 2.5, n), 12, tc=TC)
    add("y = 0", rng.normal(1.0, 0.5, 63), rng.normal(-1.0, 0.3, 63), 0)
    add("y = 0 small mean", rng.normal(-3.0, 0.5, 64), rng.normal(1.0, 0.3, 64), 0, p=P2)
    add("y = 2580228", rng.normal(14.7, 0.05, 65), rng.normal(-3.0, 0.2, 65), 2580228, tc=TC, p=P2)
    add("excluded", rng.normal(5.0, 0.3, 200), rng.normal(-1.5, 0.2, 200), 4000, excluded=True, p=P2)
    add("small counts", rng.normal(0.5, 0.4, 300), rng.normal(-0.5, 0.5, 300), 3)
    bad = rng.normal(2.0, 0.2, 50)
    bad[17] = np.nan
    add("nan eta", bad, np.full(50, -1.0), 5)
    sg = np.full(50, -1.0)
    sg[3] = np.inf                                              # phi = 0
    add("phi = 0", rng.normal(2.0, 0.2, 50), sg, 5)
    sg = np.full(50, -1.0)
    sg[49] = np.nan
    add("nan sigma", rng.normal(2.0, 0.2, 50), sg, 5, excluded=True)
    return cs


def long_columns(n, cells=5, seed=3):
    """columns at the LDS / scratch hand-over: eta [n, cells], sigma_raw [n, cells], y [cells]"""
    rng = np.random.default_rng(seed + n)
    eta = rng.normal(4.0, 0.4, (n, cells)) + np.arange(cells)[None, :] * 0.7
    sg = rng.normal(-1.0, 0.3, (n, cells))
    y = np.array([0, 40, 300, 80, 2580228][:cells])
    return eta, sg, y
