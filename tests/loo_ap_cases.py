"""Designed columns shared by tests/test_loo_ap_host.py (CPU) and tests/test_gpu_loo_ap.py (device): a cell's log-likelihood ll [n],
the draws' log ratios a = log_p - log_g [n] and whether the model excludes the cell."""
import numpy as np

from tests import loo_restate as L


def _counts(rng, n, mu=60.0, size=4.0):
    return rng.negative_binomial(size, size / (size + mu), n).astype(np.int64)


TIES = (("ties inside the tail", range(1000 - 20, 1000 - 12)),
        ("ties straddling the cutoff", range(1000 - L.tail_len(1000) - 5, 1000 - L.tail_len(1000) + 5)))


def tied(rng, ranks, n=1000):
    """(ll, a, the draws at `ranks` of the ratios a - ll): those draws share one ratio exactly and keep their ranks, inside a
    smoothed tail, while their ll differ. The shared ratio and a are short dyadic numbers, so a - ll is exact for them."""
    a = rng.integers(-6, 7, size=n) / 4.0
    r = L.P.normal_ratios(rng, 3.0, n)
    ix = np.argsort(r, kind="stable")
    ranks = list(ranks)
    lo, hi = r[ix[ranks[0] - 1]], r[ix[ranks[-1] + 1]]
    t = np.round(0.5 * (lo + hi) * 4096.0) / 4096.0
    assert lo < t < hi
    r[ix[ranks]] = t
    ll = a - r
    assert np.all((a - ll)[ix[ranks]] == t) and np.unique(ll[ix[ranks]]).size > 1
    return ll, a, ix[ranks]


def designed():
    """(name, ll, a, excluded)"""
    rng = np.random.default_rng(41)
    for n in (20, 25, 224, 1000, 4000):                                    # n = 20: M = 4, khat = +Inf
        for s in (0.3, 1.0, 2.5):
            yield f"normal ll n={n} s={s}", -L.P.normal_ratios(rng, 3.0, n), rng.normal(0.0, s, n), False
            yield f"gpd ll n={n} s={s}", -np.log(L.P.gpd_sample(rng, 0.7, n)), rng.normal(0.0, s, n), False
    # tied ratios with different ll: who gets which smoothed weight matters
    yield "ties, different ll", rng.poisson(3.0, size=1000).astype(float), rng.poisson(4.0, size=1000).astype(float), False
    yield "ties, different ll, excluded", rng.poisson(3.0, size=1000).astype(float), rng.poisson(4.0, size=1000).astype(float), True
    for name, ranks in TIES:                                               # ... within a smoothed tail
        ll, a, _ = tied(rng, ranks)
        yield name, ll, a, False
    a = rng.integers(-4, 5, size=1000) / 2.0
    ll = a - np.concatenate([rng.normal(size=900), np.full(100, 5.0)])     # a - ll = 5 exactly at the last 100 draws
    yield "constant tail", ll, a, False
    a = rng.normal(0.0, 1.0, 1000)
    a[::7] = -np.inf                                                       # log_p not finite: the draw takes no part
    yield "-inf a takes no part", rng.normal(size=1000), a, False
    yield "-inf a takes no part, excluded", rng.normal(size=1000), a, True
    ll = rng.normal(size=1000)
    ll[::9] = np.inf
    yield "+inf ll takes no part", ll, rng.normal(0.0, 1.0, 1000), False
    yield "+inf ll excluded", ll, rng.normal(0.0, 1.0, 1000), True
    ll = rng.normal(size=1000)
    ll[5] = -np.inf
    yield "-inf ll", ll, rng.normal(0.0, 1.0, 1000), False
    yield "-inf ll excluded", ll, rng.normal(0.0, 1.0, 1000), True         # an ordinary draw: its term is 0
    a = rng.normal(0.0, 1.0, 500)
    a[9] = np.nan
    yield "nan a", rng.normal(size=500), a, False
    yield "nan a excluded", rng.normal(size=500), a, True
    ll = rng.normal(size=500)
    ll[9] = np.nan
    yield "nan ll", ll, rng.normal(0.0, 1.0, 500), False
    yield "nan ll excluded", ll, rng.normal(0.0, 1.0, 500), True
    yield "no draw takes part", rng.normal(size=300), np.full(300, -np.inf), False
    for n in (25, 2000):
        yield f"excluded n={n}", rng.normal(-3.0, 0.7, size=n), L.P.normal_ratios(rng, 2.0, n), True
    yield "far from zero", -L.P.normal_ratios(rng, 5.0, 4000) - 1.0e4, rng.normal(-3.0e3, 2.0, 4000), False


def predictive():
    """(name, ll, a, x, y, excluded, p_lo, p_hi): the columns above with predictive counts, and ties whose counts differ"""
    rng = np.random.default_rng(43)
    for name, ll, a, excluded in designed():
        if ll.size >= 224:
            yield name, ll, a, _counts(rng, ll.size), 55, excluded, 0.025, 0.975
    for name, ranks in TIES:
        ll, a, who = tied(rng, ranks)
        x = _counts(rng, 1000)
        x[who] = np.array([0, 5000, 3, 900, 20000, 1, 7000, 12, 15000, 2])[:who.size]   # who gets which weight matters
        yield name + ", counts differ", ll, a, x, 60, False, 0.05, 0.95
    x = _counts(rng, 500)
    x[77] = 2147483647
    yield "invalid draw", rng.normal(size=500), rng.normal(size=500), x, 40, False, 0.025, 0.975
    yield "excluded, p = 0 / 1", rng.normal(size=300), L.P.normal_ratios(rng, 2.0, 300), _counts(rng, 300), 50, True, 0.0, 1.0


def long_columns(n, n_cols=7, seed=9):
    """smooth columns of n draws (the LDS path's last length, the scratch path's first, a long one), the last one excluded"""
    rng = np.random.default_rng(seed + n)
    ll = np.stack([-L.P.normal_ratios(rng, 2.5, n) for _ in range(n_cols)], axis=1)
    x = np.stack([_counts(rng, n) for _ in range(n_cols)], axis=1)
    excl = np.zeros(n_cols, np.int32)
    excl[-1] = 1
    return ll, L.P.normal_ratios(rng, 1.8, n), x, np.full(n_cols, 58), excl
