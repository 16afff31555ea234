"""Designed columns shared by tests/test_loo_exact_host.py (CPU) and tests/test_gpu_loo_exact.py (device): the ratio columns of
tests/loo_predict_cases.designed() (and, for the ADVI form, of tests/loo_ap_cases.designed()), each with its own linear
predictors eta [n], sigma_raw [n] and observed count y in the style of tests/ppc_exact_restate.designed(); then the pass-2
probabilities and truncation compensation, a draw with invalid parameters, weights that follow mu, p_lo = 0 and a refused
p_hi."""
import numpy as np

from tests import loo_ap_cases
from tests import loo_predict_cases
from tests import loo_restate as L
from tests.ppc_exact_restate import P2, TC

RATIO_COLUMNS = ("smooth tail n=1000", "smooth tail n=3000", "smooth tail n=4000", "r_eff 0.3", "heavy tail", "M < 5", "constant tail",
                 "constant column", "+inf ll takes no part", "-inf ll", "-inf ll excluded", "nan ll", "nan ll excluded",
                 "ties everywhere", "ties inside the tail", "ties straddling the cutoff", "ties from the cutoff up")
AP_COLUMNS = ("normal ll n=224 s=1.0", "gpd ll n=1000 s=2.5", "normal ll n=4000 s=0.3", "ties, different ll", "ties, different ll, excluded",
              "ties inside the tail", "ties straddling the cutoff", "constant tail", "-inf a takes no part",
              "-inf a takes no part, excluded", "+inf ll takes no part", "+inf ll excluded", "-inf ll", "-inf ll excluded", "nan a",
              "nan ll excluded", "no draw takes part", "excluded n=2000")


def _tied(v):
    """mask of the draws whose value occurs more than once"""
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    return cnt[inv] > 1


def designed():
    """dicts of name, ll [n], eta [n], sg [n] (sigma_raw), y, lr (None, or [n]: the log ratios of an ADVI fit), r_eff, excluded,
    tc, p_lo, p_hi and `refused`: the probabilities are ones the entry points refuse (the header itself takes p_lo = 0)."""
    rng = np.random.default_rng(57)
    cs = []

    def add(name, ll, eta, sg, y, lr=None, r_eff=1.0, excluded=False, tc=1.0, p_lo=0.025, p_hi=0.975, refused=False):
        cs.append(dict(name=name, ll=np.asarray(ll, np.float64), eta=np.asarray(eta, np.float64), sg=np.asarray(sg, np.float64), y=int(y),
                       lr=None if lr is None else np.asarray(lr, np.float64), r_eff=r_eff, excluded=excluded, tc=tc, p_lo=p_lo,
                       p_hi=p_hi, refused=refused))

    def columns(n, tied=None):
        eta, sg = rng.normal(4.0, 0.5, n), rng.normal(-1.0, 0.3, n)
        if tied is not None and tied.any() and not tied.all():   # who gets which weight matters: the tied draws differ widely
            eta[tied] = np.resize(np.array([1.0, 7.5, 2.0, 6.5, 9.0, 0.5, 7.0, 3.0, 8.5, 1.5]), int(tied.sum()))
        return eta, sg

    by = {c["name"]: c for c in loo_predict_cases.designed()}
    for k, name in enumerate(RATIO_COLUMNS):
        c = by[name]
        n = c["ll"].size
        tied = _tied(c["ll"]) if name.startswith("ties") else None
        eta, sg = columns(n, tied)
        pass2 = k % 3 == 1                                        # every third column at the pass-2 settings
        add(name, c["ll"], eta, sg, (0, 40, 300, 80)[k % 4], r_eff=c["r_eff"], excluded=c["excluded"], tc=TC if pass2 else 1.0,
            p_lo=P2 if pass2 else 0.025, p_hi=1 - P2 if pass2 else 0.975)
    ap = {name: (ll, a, excluded) for name, ll, a, excluded in loo_ap_cases.designed()}
    for k, name in enumerate(AP_COLUMNS):
        ll, a, excluded = ap[name]
        n = ll.size
        r = a if excluded else a - ll
        tied = _tied(r) if name.startswith("ties") else None
        eta, sg = columns(n, tied)
        pass2 = k % 3 == 2
        add("advi: " + name, ll, eta, sg, (55, 0, 120, 30)[k % 4], lr=a, excluded=excluded, tc=TC if pass2 else 1.0,
            p_lo=P2 if pass2 else 0.025, p_hi=1 - P2 if pass2 else 0.975)
    # ---- the predictive side
    n = 2000
    eta, sg = rng.normal(6.5, 0.3, n), rng.normal(-2.0, 0.2, n)
    add("pass 2", -L.P.normal_ratios(rng, 2.0, n), eta, sg, 900, tc=TC, p_lo=P2, p_hi=1 - P2)
    add("pass 2, excluded", -L.P.normal_ratios(rng, 2.0, n), eta, sg, 900, excluded=True, tc=TC, p_lo=P2, p_hi=1 - P2)
    add("pass 2, advi", -L.P.normal_ratios(rng, 2.0, n), eta, sg, 900, lr=rng.normal(0.0, 1.0, n), tc=TC, p_lo=P2, p_hi=1 - P2)
    add("y = 2580228", -L.P.normal_ratios(rng, 1.5, 65), rng.normal(14.7, 0.05, 65), rng.normal(-3.0, 0.2, 65), 2580228, tc=TC, p_lo=P2,
        p_hi=1 - P2)
    add("one draw", [-3.0], [4.2], [-1.3], 60)
    for name, i, what in (("nan eta", 17, "eta"), ("phi = 0", 3, "sg"), ("nan sigma, excluded", 49, "sg")):
        eta, sg = rng.normal(2.0, 0.2, 50), np.full(50, -1.0)
        (eta if what == "eta" else sg)[i] = np.inf if name == "phi = 0" else np.nan
        add(name, rng.normal(-3.0, 1.0, 50), eta, sg, 5, excluded=name.endswith("excluded"))
    # weights that follow mu: the draws with a large mean fit the cell badly, so holding the cell out moves the interval up
    n = 2000
    eta, sg = rng.normal(5.0, 0.5, n), rng.normal(-1.0, 0.1, n)
    add("weights follow mu", -1.5 * (eta - 5.0) + rng.normal(0.0, 0.2, n), eta, sg, 60, p_lo=0.05, p_hi=0.95)
    eta, sg = rng.normal(3.0, 0.4, 1000), rng.normal(-0.5, 0.3, 1000)
    add("p_lo = 0", -L.P.normal_ratios(rng, 2.0, 1000), eta, sg, 20, p_lo=0.0, p_hi=0.9, refused=True)
    add("p_hi = 1", -L.P.normal_ratios(rng, 2.0, 1000), eta, sg, 20, p_lo=0.1, p_hi=1.0, refused=True)
    return cs


def long_columns(n, cells=5, seed=3):
    """columns at the ends of the workgroup's stride and at the LDS / scratch hand-over: ll, eta, sigma_raw [n, cells], y [cells],
    excluded [cells] (the last cell), r_eff [cells], and lr [n] for the ADVI form"""
    rng = np.random.default_rng(seed + n)
    ll = np.stack([-L.P.normal_ratios(rng, 2.5, n) for _ in range(cells)], axis=1)
    eta = rng.normal(4.0, 0.4, (n, cells)) + np.arange(cells)[None, :] * 0.7
    sg = rng.normal(-1.0, 0.3, (n, cells))
    y = np.array([0, 40, 300, 80, 2580228][:cells])
    excl = np.zeros(cells, np.int32)
    excl[-1] = 1
    return ll, eta, sg, y, excl, np.linspace(0.4, 1.0, cells), L.P.normal_ratios(rng, 1.8, n)
