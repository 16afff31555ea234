"""Inputs shared by tests/test_loo_predict_host.py (CPU) and tests/test_gpu_loo_predict.py (device): designed columns for
the leave-one-out predictive interval (ties, cutoff copies, degenerate tails) and the inputs of the fit test -- the oracle's NUTS
draws on a small problem, scipy's log-likelihood and the oracle's predictive counts at the product's Philox address."""
import math

import numpy as np

from tests import loo_restate as L

FIT_EXCL = (3, 17)                # excluded cells (g S + s) of the fit test
FIT_SEED = 5                      # of the predictive draws


def _counts(rng, n, mu=60.0, size=4.0):
    return rng.negative_binomial(size, size / (size + mu), n).astype(np.int64)


def designed():
    """dicts of name, ll [n], x [n], y, r_eff, excluded, p_lo, p_hi; `exact_upper`: the upper quantile sits on F = p by
    construction (p_hi = 1) and is compared without the borderline skip (v* is the largest drawn value either way)."""
    rng = np.random.default_rng(31)
    out = []

    def add(name, ll, x, y, r_eff=1.0, excluded=False, p_lo=0.025, p_hi=0.975, **kw):
        out.append(dict(name=name, ll=np.asarray(ll, float), x=np.asarray(x, np.int64), y=int(y), r_eff=r_eff,
                        excluded=excluded, p_lo=p_lo, p_hi=p_hi, **kw))

    for n, s2 in ((1000, 1.5), (3000, 3.0), (4000, 10.0)):
        add(f"smooth tail n={n}", -L.P.normal_ratios(rng, s2, n), _counts(rng, n), 55)
    add("r_eff 0.3", -L.P.normal_ratios(rng, 2.0, 2000), _counts(rng, 2000), 10, r_eff=0.3)
    add("heavy tail", -np.log(L.P.gpd_sample(rng, 0.8, 3000)), _counts(rng, 3000), 400)
    # weights that follow the counts: the held-out interval moves away from y
    x = _counts(rng, 2000)
    add("weights follow the counts", -0.02 * np.abs(x - 300.0) + rng.normal(0, 0.3, 2000), x, 300, p_lo=0.05, p_hi=0.95)
    add("M < 5", rng.normal(size=20), _counts(rng, 20), 30)
    add("constant tail", -np.concatenate([rng.normal(size=900), np.full(100, 5.0)]), _counts(rng, 1000), 70)
    add("constant column", np.full(500, -2.5), _counts(rng, 500), 70)
    ll = rng.normal(size=1000); ll[::7] = np.inf
    add("+inf ll takes no part", ll, _counts(rng, 1000), 40)
    ll = rng.normal(size=1000); ll[5] = -np.inf
    add("-inf ll", ll, _counts(rng, 1000), 40)
    add("-inf ll excluded", ll, _counts(rng, 1000), 40, excluded=True)
    ll = rng.normal(size=500); ll[9] = np.nan
    add("nan ll", ll, _counts(rng, 500), 40)
    add("nan ll excluded", ll, _counts(rng, 500), 40, excluded=True)
    x = _counts(rng, 500); x[77] = 2147483647
    add("invalid draw", rng.normal(size=500), x, 40)
    # ---- ties in the ratios with different counts
    add("ties everywhere", -rng.poisson(3.0, size=1000).astype(float), _counts(rng, 1000), 60)
    n = 1000
    M = L.tail_len(n)
    for name, ranks in (("ties inside the tail", range(n - 20, n - 12)), ("ties straddling the cutoff", range(n - M - 5, n - M + 5)),
                        ("ties from the cutoff up", range(n - M - 1, n - M + 6))):
        r = L.P.normal_ratios(rng, 3.0, n)
        ix = np.argsort(r, kind="stable")
        ranks = list(ranks)
        r[ix[ranks]] = 0.5 * (r[ix[ranks[0] - 1]] + r[ix[ranks[-1] + 1]])     # they keep their ranks, as one value
        x = _counts(rng, n)
        x[ix[ranks]] = np.array([0, 5000, 3, 900, 20000, 1, 7000, 12, 15000, 2])[:len(ranks)]   # who gets which weight matters
        add(name, -r, x, 60)
    add("all counts equal", -L.P.normal_ratios(rng, 2.0, 1000), np.full(1000, 7), 7)
    add("p_lo = 0, p_hi = 1", -L.P.normal_ratios(rng, 2.0, 1000), _counts(rng, 1000), 60, p_lo=0.0, p_hi=1.0, exact_upper=True)
    x = _counts(rng, 2000, mu=3.0, size=0.5)                                  # a third of the draws are 0
    add("v* at the smallest drawn value", -L.P.normal_ratios(rng, 2.0, 2000), x, 0)
    x = np.where(rng.uniform(size=2000) < 0.05, 500, _counts(rng, 2000, mu=20.0))
    add("v* at the largest drawn value", -L.P.normal_ratios(rng, 2.0, 2000), np.minimum(x, 500), 500, p_lo=0.01, p_hi=0.999)
    for n in (7, 1000, 2001):
        add(f"excluded n={n}", rng.normal(-3.0, 0.7, size=n), _counts(rng, n), 50, excluded=True, p_lo=0.05, p_hi=0.95)
    add("excluded, odd probabilities", rng.normal(size=999), _counts(rng, 999), 50, excluded=True, p_lo=0.0017, p_hi=0.9983)
    add("excluded p = 0 / 1", rng.normal(size=300), _counts(rng, 300), 50, excluded=True, p_lo=0.0, p_hi=1.0)
    return out


def long_columns(n, n_cols=7, seed=9):
    """smooth columns of n draws (the LDS path's last length, the scratch path's first, a long one)"""
    rng = np.random.default_rng(seed + n)
    ll = np.stack([-L.P.normal_ratios(rng, 2.5, n) for _ in range(n_cols)], axis=1)
    x = np.stack([_counts(rng, n) for _ in range(n_cols)], axis=1)
    return ll, x, np.full(n_cols, 58)


def params(draws, G, C, K):
    """alpha [n, C, G] and sigma_raw [n, G] at each draw (oracle.independent.unpack)"""
    from oracle.independent import unpack
    n = draws.shape[0]
    alpha, sr = np.zeros((n, C, G)), np.zeros((n, G))
    for i in range(n):
        p = unpack(draws[i], G, C, K, 5.612671)
        alpha[i, 0] = p["intercept"]
        if C >= 2:
            alpha[i, 1, :K] = p["alpha1"]
        if C >= 3:
            alpha[i, 2:, :K] = p["alpha2"]
        sr[i] = p["sigma_raw"]
    return alpha, sr


def predictive_counts(oracle, draws, X, expo, K, seed, tc=1.0):
    """x [n, G, S]: the oracle's neg_binomial_2_log_rng(eta, tc exp(-sigma_raw)) at the address (seed, g S + s, draw) for ALL
    genes (eta accumulated as the oracle's generated quantities accumulate it)."""
    n = draws.shape[0]
    S, C = X.shape
    alpha, sr = params(draws, (draws.shape[1] - 6 - K * (C - 1)) // 2, C, K)
    G = sr.shape[1]
    x = np.zeros((n, G, S), np.int64)
    for i in range(n):
        for g in range(G):
            phi = math.exp(-sr[i, g]) * tc
            for s in range(S):
                eta = expo[s] + X[s, 0] * alpha[i, 0, g]
                for c in range(1, C):
                    eta += X[s, c] * alpha[i, c, g]
                x[i, g, s] = oracle.nb2_log_rng(eta, phi, seed, g * S + s, i)
    return x


_FIT = {}


def fit_inputs(oracle):
    """The fit test's inputs, without a GPU: dict of d (synth(30, 10, K = 4, seed = 5)), draws [4, 250, D] of the oracle's NUTS with
    the cells FIT_EXCL excluded, ll [1000, 30, 10] (scipy) and x [1000, 30, 10] (the oracle's counts at seed FIT_SEED)."""
    if not _FIT:
        from ppcseq_amd.synth import synth
        d = synth(30, 10, K=4, seed=5)
        excl = np.array(FIT_EXCL, np.int32)
        mo = oracle.model(d["counts"], d["X"], d["exposure"], 4, excl=excl, n_threads=4)
        r = oracle.nuts_model(mo, oracle.cfg(chains=4, iter=400, warmup=150, seed=3))
        draws = r.draws
        flat = draws.reshape(-1, draws.shape[-1])
        X = np.asarray(d["X"], float)
        alpha, sr = params(flat, 30, 2, 4)
        eta = np.einsum("sc,ncg->ngs", X, alpha) + d["exposure"][None, None, :]
        ll = L.log_lik(d["counts"][None], eta, sr[:, :, None])
        x = predictive_counts(oracle, flat, X, d["exposure"], 4, FIT_SEED)
        _FIT.update(d=d, draws=draws, ll=ll, x=x, excl=excl)
    return _FIT
