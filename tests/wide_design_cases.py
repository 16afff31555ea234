"""Designed draws of designs with more than one slope, shared by tests/test_wide_designs_host.py (CPU) and
tests/test_gpu_wide_designs.py (device): three genes (two checked, one not: K = 2, so the alpha2 block holds the further slopes
of two genes side by side and a wrong stride reads the other gene's) on

    "covariate"  C = 3, S = 6: ones, a 0/1 group and a centred continuous covariate; one excluded cell in gene 0's row
    "factor4"    C = 4, S = 8: ones and three indicators; one excluded cell in gene 1's row

The product grid of tests/loo_mm_cases.py does not reach d = 4 or 5 coordinates, so a gene's draws come from n independent
random-walk Metropolis chains, one per draw, on the restatement's own density (tests/loo_mm_restate.local_density) at HYPER; the
draws' hyper-parameters carry the jitter of loo_mm_cases.tiny_set. A draw set is the dict of tests/loo_mm_cases.py and
loo_mm_cases.gene_of() cuts a gene out of it."""
import numpy as np

from tests.loo_mm_cases import HYPER, LAMBDA_MU_MU, dims, slope_index

G, K = 3, 2

# The largest errors measured on these cells, in units of max(1, |ref|) (the statistics' own errors() functions). WIDE_MEASURED:
# the CPU builds against the restatements (tests/test_wide_designs_host.py prints them); WIDE_GPU_MEASURED: the device against
# the CPU builds (tests/test_gpu_wide_designs.py prints them). A comparison's bound is ten times its value, never above BOUND.
BOUND = 1e-9
WIDE_MEASURED = dict(mm=3.0e-11, exact=3.0e-11, split=5.1e-11, density=1.4e-11)     # 2.95e-11, 2.95e-11, 5.01e-11, 1.37e-11
WIDE_GPU_MEASURED = dict(mm=1.4e-11, split=2.7e-11, exact=1.4e-11, exact_split=2.7e-11,         # 1.38e-11, 2.68e-11, twice
                         counts=1.8e-11)                                                      # 1.75e-11 at n = 1000


def metropolis(rng, n, y, excl, expo, X, checked, steps=300, sd=0.25):
    """T [C + 1, n]: the state of n independent chains after `steps` random-walk steps of sd `sd` on the gene's coordinates from
    (log median y, 0, .., 0, -1), targeting the gene's posterior given HYPER; a row that is no coordinate of the gene stays 0"""
    from tests import loo_mm_restate as R
    Cc = X.shape[1]
    nc = Cc + 1
    T = np.zeros((nc, n))
    T[0], T[Cc] = np.log(max(np.median(y), 1.0)), -1.0
    use = np.array([c == 0 or c == Cc or checked for c in range(nc)], np.float64)
    U = np.repeat(HYPER[:, None], n, axis=1)

    def q(t):
        gene = dict(T=t, U=U, y=y, excl=excl, expo=expo, X=X, checked=checked, lambda_mu_mu=LAMBDA_MU_MU)
        return R.local_density(gene, np.ones(nc), np.zeros(nc))[0]

    cur = q(T)
    for _ in range(steps):
        P = T + use[:, None] * rng.normal(0.0, sd, (nc, n))
        qp = q(P)
        ok = np.log(rng.uniform(size=n)) < qp - cur
        T[:, ok], cur[ok] = P[:, ok], qp[ok]
    return T


X3 = np.array([[1, 0, -1.35], [1, 1, 0.15], [1, 0, 0.65], [1, 1, -0.65], [1, 0, 1.25], [1, 1, -0.05]], np.float64)
X4 = np.array([[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [1, 0, 0, 0]], np.float64)

# gene 0: a group effect upwards and one count of 2 500; gene 1: other slopes (downwards) and an outlier of its own; gene 2
# (not checked): one low outlier among level counts
SPECS = {
    "covariate": dict(X=X3, seed=21, excl=((0, 2),),
                      counts=[[120, 180, 95, 160, 140, 2500], [400, 90, 2200, 110, 640, 150], [300, 2, 330, 310, 290, 305]]),
    "factor4": dict(X=X4, seed=22, excl=((1, 3),),
                    counts=[[120, 180, 95, 160, 140, 2500, 130, 150], [300, 80, 520, 210, 95, 30, 190, 310],
                            [300, 2, 330, 310, 290, 305, 320, 295]]),
}


def wide_set(name, n=1000, seed=None, hyper_jitter=0.02):
    spec = SPECS[name]
    seed = spec["seed"] if seed is None else seed
    X = spec["X"]
    S, Cc = X.shape
    counts = np.asarray(spec["counts"], np.int32)
    assert counts.shape == (G, S)
    expo = np.linspace(-0.1, 0.1, S)
    excl = np.zeros((G, S), bool)
    for g, s in spec["excl"]:
        excl[g, s] = True
    d = dims(G, Cc, K)
    u = np.zeros((n, d["D"]))
    h = HYPER[None, :] + np.random.default_rng(seed).normal(0.0, hyper_jitter, (n, 6))
    u[:, 0:3], u[:, d["tail"]:d["tail"] + 3] = h[:, :3], h[:, 3:]
    for g in range(G):
        T = metropolis(np.random.default_rng([seed, g]), n, counts[g], excl[g], expo, X, g < K)
        u[:, d["intercept"] + g], u[:, d["sigma_raw"] + g] = T[0], T[Cc]
        if g < K:
            for c in range(1, Cc):
                u[:, slope_index(d, Cc, c, g)] = T[c]
    return dict(counts=counts, X=X, expo=expo, K=K, excl=np.flatnonzero(excl.ravel()).astype(np.int32), lambda_mu_mu=LAMBDA_MU_MU,
                draws=u)


_SETS = {}


def draw_set(name):
    """ "covariate" and "factor4" at 1 000 draws; "long": "factor4" at 4 097 draws (its prefixes are the draw counts of the
    device test). Built once."""
    if name not in _SETS:
        _SETS[name] = wide_set("factor4", n=4097, seed=23) if name == "long" else wide_set(name)
    return _SETS[name]


def designed():
    """dicts of name, set, g, s, r_eff, k_threshold, max_iters and `kinds`, as tests/loo_mm_cases.designed() gives them"""
    cs = []

    def add(name, set_, g, s, kinds, r_eff=1.0, k_threshold=0.7, max_iters=30):
        cs.append(dict(name=name, set=set_, g=g, s=s, kinds=kinds, r_eff=r_eff, k_threshold=k_threshold, max_iters=max_iters))

    add("covariate: repeated shifts at the outlier (d = 4)", "covariate", 0, 5, [1, 1, 1])
    add("covariate: shift, then shift and scale (d = 4)", "covariate", 0, 4, [1, 2], k_threshold=0.5)
    add("covariate: gene 1, shifts, then shift and scale", "covariate", 1, 0, [1, 1, 2], k_threshold=0.5)
    add("covariate: gene 1's outlier", "covariate", 1, 2, [1])
    add("covariate: r_eff = 0.4", "covariate", 0, 3, None, r_eff=0.4)
    add("covariate: outlier in the unchecked gene", "covariate", 2, 1, [1])
    add("covariate: excluded cell", "covariate", 0, 2, [])
    add("covariate: below the threshold", "covariate", 1, 1, [])
    add("factor4: one shift (d = 5)", "factor4", 0, 2, [1])
    add("factor4: shift and scale first (d = 5)", "factor4", 1, 6, [2, 1, 1])
    add("factor4: shift and scale alone", "factor4", 0, 3, [2], k_threshold=0.5)
    add("factor4: nine steps", "factor4", 0, 6, [1] * 8 + [2], k_threshold=0.5)
    add("factor4: khat stays above the threshold", "factor4", 0, 5, [1])
    add("factor4: stops at max_iters", "factor4", 1, 2, [1, 1], max_iters=2)
    add("factor4: outlier in the unchecked gene", "factor4", 2, 1, [1])
    add("factor4: excluded cell", "factor4", 1, 3, [])
    add("factor4: below the threshold", "factor4", 0, 0, [])
    return cs


def columns(ds, col):
    """eta [n, G, S] and sigma_raw [n, G] of every gene in numpy, for any C: col(indices) gives those columns of the draws
    [n, len(indices)] (the draw set's own array on the CPU, Fit.columns on the device). A gene that is not checked has no slopes."""
    X, expo = np.asarray(ds["X"], np.float64), np.asarray(ds["expo"], np.float64)
    S, Cc = X.shape
    n_genes, k = ds["counts"].shape[0], ds["K"]
    d = dims(n_genes, Cc, k)
    eta = expo[None, None, :] + col(d["intercept"] + np.arange(n_genes))[:, :, None] * X[None, None, :, 0]
    for c in range(1, Cc):
        a = col(np.array([slope_index(d, Cc, c, g) for g in range(k)]))
        eta[:, :k, :] += a[:, :, None] * X[None, None, :, c]
    return eta, col(d["sigma_raw"] + np.arange(n_genes))
