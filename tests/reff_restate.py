"""numpy restatement of the relative efficiency per cell (include/ppcx.h ppcx_fit_relative_eff, ppcseq_amd/csrc/ppcx_reff.h):
loo::relative_eff(exp(log_lik), chain_id) as posterior::ess_mean over the split chains, on v = exp(ll - max ll). Built from
tests/summary_restate.py's split and Geyer ESS. Shared by tests/test_reff_host.py (CPU) and tests/test_gpu_reff.py (device)."""
import numpy as np

from tests import summary_restate as R


def relative_eff(ll):
    """ll [M, n] (a cell's log-likelihoods by chain) -> r_eff"""
    ll = np.asarray(ll, dtype=np.float64)
    M, n = ll.shape
    if n // 2 < 2:
        return float("nan")
    sp = R.split(ll)
    if np.any(np.isnan(sp)) or np.any(sp == np.inf):
        return float("nan")
    L = sp.max()
    if L == -np.inf:                              # every value -Inf: all equal
        return float("nan")
    return R.ess_seq(np.exp(sp - L)) / sp.size


def relative_eff_columns(ll, chains):
    """ll [chains * n, n_cells], draws chain-major -> [n_cells]"""
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(ll.shape[0], -1)
    return np.array([relative_eff(ll[:, c].reshape(chains, -1)) for c in range(ll.shape[1])])


# ---- the columns both checks run

SHAPES = ((1, 4), (1, 5), (2, 11), (4, 64), (4, 250))


def ar1(rng, phi, M, n, sd=1.0):
    """M chains of n draws of a stationary AR(1) with lag-one correlation phi and marginal standard deviation sd"""
    x = np.empty((M, n))
    x[:, 0] = rng.normal(size=M)
    e = rng.normal(size=(M, n)) * np.sqrt(1 - phi * phi)
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return sd * x


def seeded_cases():
    """(name, ll [M, n]) of the seeded columns at every shape. The seed was chosen after checking that no case has a Geyer pair
    sum within 1e-9 of zero at its truncation (rounding would flip it), with the restatement alone."""
    for M, n in SHAPES:
        rng = np.random.default_rng(1000 * M + n)
        yield f"iid M={M} n={n}", rng.normal(-3.0, 0.7, size=(M, n))
        yield f"ar1 0.5 M={M} n={n}", -3.0 + ar1(rng, 0.5, M, n, 0.7)
        yield f"ar1 0.9 M={M} n={n}", -3.0 + ar1(rng, 0.9, M, n, 0.7)
        yield f"antithetic M={M} n={n}", -3.0 + ar1(rng, -0.5, M, n, 0.7)
        x = rng.normal(-3.0, 0.7, size=(M, n))
        x[M - 1] += 1.5                                                  # one chain shifted against the others
        yield f"shifted chain M={M} n={n}", x


def rule_cases():
    """(name, ll [M, n], expectation: "nan" or "finite")"""
    rng = np.random.default_rng(77)
    yield "constant", np.full((4, 64), -2.5), "nan"
    x = rng.normal(size=(4, 64)); x[1, 3] = np.nan
    yield "nan", x, "nan"
    x = rng.normal(size=(4, 64)); x[2, 40] = np.inf
    yield "+inf", x, "nan"
    x = rng.normal(size=(4, 64)); x[0, 5] = x[3, 60] = -np.inf
    yield "-inf", x, "finite"
    yield "all -inf", np.full((2, 11), -np.inf), "nan"
    yield "n = 3", rng.normal(size=(2, 3)), "nan"
    x = rng.normal(size=(2, 5)); x[:, 2] = np.nan                       # an odd n drops the middle draw, whatever it holds
    yield "nan in the dropped draw", x, "finite"


def min_pair_margin(ll):
    """the smallest |even + odd| the Geyer recurrence of this cell compares with zero (the seeds' check)"""
    sp = R.split(np.asarray(ll, dtype=np.float64))
    z = np.exp(sp - sp.max())
    m, nh = z.shape
    c = z - z.mean(axis=1, keepdims=True)
    acov = lambda t: np.mean(np.sum(c[:, :nh - t] * c[:, t:], axis=1) / nh)
    mv = acov(0) * nh / (nh - 1)
    vp = mv * (nh - 1) / nh + z.mean(axis=1).var(ddof=1)
    rho = lambda t: 1 - (mv - acov(t)) / vp
    t, even, odd, mn = 0, 1.0, rho(1), np.inf
    while t < nh - 5 and even + odd > 0:
        t += 2
        even, odd = rho(t), rho(t + 1)
        mn = min(mn, abs(even + odd))
    return mn
