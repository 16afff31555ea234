"""Designed draws of designs with more than one slope, shared by tests/test_wide_designs_host.py (CPU) and
tests/test_gpu_wide_designs.py (device): three genes (two checked, one not: K = 2, so the alpha2 block holds the further slopes
of two genes side by side and a wrong stride reads the other gene's) on

    "covariate"  C = 3, S = 6: ones, a 0/1 group and a centred continuous covariate; one excluded cell in gene 0's row
    "factor4"    C = 4, S = 8: ones and three indicators; one excluded cell in gene 1's row

and, for tests/test_widest_designs_host.py and tests/test_gpu_widest_designs.py, on the widest designs the library takes

    "columns8"   C = 8, S = 12: ones, six indicators and a centred continuous covariate; one excluded cell in gene 1's row
    "columns16"  C = 16, S = 20: ones and fifteen indicators, the first levels twice; one excluded cell in gene 1's row
    "columns15"  "columns16" cut down to its first 15 columns: (C + 1)^2 = 256

The product grid of tests/loo_mm_cases.py does not reach d = 4 or more coordinates, so a gene's draws come from n independent
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
# The same on the cells of "columns8", "columns16" and "columns15" (designed(widest=True), loo_mm_cov_cases.designed(widest=True)),
# one value per statistic and width. WIDEST_MEASURED: tests/test_widest_designs_host.py prints them (`cov`: the covariance form on
# its designed cells, split both ways; `counts`: on the draw-count cells); WIDEST_GPU_MEASURED: tests/test_gpu_widest_designs.py.
WIDEST_MEASURED = dict(columns8=dict(mm=5.2e-11, exact=8.1e-11, split=5.7e-11, cov=9.0e-11, counts=8.7e-12),     # 5.12e-11, 8.02e-11, 5.62e-11, 8.95e-11, 8.66e-12 (n = 257)
                       columns16=dict(mm=2.8e-11, exact=2.8e-11, split=3.7e-11, cov=2.2e-10, counts=4.3e-11),    # 2.76e-11, 2.76e-11, 3.67e-11, 2.197e-10, 4.29e-11 (n = 255)
                       columns15=dict(cov=2.2e-11))                                                              # 2.194e-11
WIDEST_GPU_MEASURED = dict(
    columns8=dict(mm=1.6e-11, split=1.6e-11, exact=2.6e-11, exact_split=1.5e-11, cov=5.5e-11, diag=1.4e-13,      # 1.599e-11 twice, 2.506e-11, 1.442e-11, 5.43e-11, 1.34e-13
                  counts=1.4e-11),                                                                               # 1.32e-11 at n = 257
    columns16=dict(mm=2.6e-11, split=3.0e-11, exact=2.6e-11, exact_split=2.6e-11, cov=4.9e-11, diag=4.8e-13,     # 2.513e-11, 2.995e-11, 2.513e-11 twice, 4.88e-11, 4.74e-13
                   counts=2.1e-11),                                                                              # 2.08e-11 at n = 257
    columns15=dict(cov=9.2e-12, diag=3.1e-14))                                                                   # 9.19e-12, 3.03e-14


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


# ---- the widest designs (tests/test_widest_designs_host.py, tests/test_gpu_widest_designs.py): C = 8 with a continuous covariate
# (the generic constants path; the widest design that may hold one) and C = 16 (kMaxC: ones and fifteen indicators). Sample s sits
# in level s % C (level 0: the ones alone), so with S > C + 1 samples the first levels occur twice and a slope is not determined by
# a single cell. Counts from 80..400, on them the outliers of the narrower sets: 2 500 in gene 0, 2 200 in gene 1, 2 in gene 2.
COV8 = (-1.35, 0.15, 0.65, -0.65, 1.25, -0.05, 0.85, -0.95, 0.45, -0.25, 1.05, -1.15)      # centred, no integer among them


def indicator_design(S, Cc):
    X = np.zeros((S, Cc))
    X[:, 0] = 1.0
    for s in range(S):
        if s % Cc:
            X[s, s % Cc] = 1.0
    return X


def _widest_counts(seed, S):
    y = np.random.default_rng(seed).integers(80, 401, (G, S))
    y[0, 5], y[1, 2], y[2, 1] = 2500, 2200, 2
    return y.tolist()


X8 = indicator_design(12, 8)
X8[:, 7] = COV8
X16 = indicator_design(20, 16)
SPECS["columns8"] = dict(X=X8, seed=24, excl=((1, 3),), counts=_widest_counts(124, 12))
SPECS["columns16"] = dict(X=X16, seed=25, excl=((1, 3),), counts=_widest_counts(128, 20))
WIDEST = ("columns8", "columns16")


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


def cut_columns(ds, Cc):
    """the draw set on the first Cc columns of its design: the same counts, hyper-parameters, intercepts, first Cc - 1 slopes and
    sigma_raw, laid out as a Cc-column model has them. An indicator design stays one: a sample of a level that is cut joins
    level 0. The draws are not a posterior sample of the narrower model; the statistics take any draws."""
    n_genes, k = ds["counts"].shape[0], ds["K"]
    C0 = ds["X"].shape[1]
    assert 2 <= Cc <= C0
    d0, d1 = dims(n_genes, C0, k), dims(n_genes, Cc, k)
    u0 = ds["draws"]
    u = np.zeros((u0.shape[0], d1["D"]))
    u[:, 0:3], u[:, d1["tail"]:d1["tail"] + 3] = u0[:, 0:3], u0[:, d0["tail"]:d0["tail"] + 3]
    for g in range(n_genes):
        u[:, d1["intercept"] + g], u[:, d1["sigma_raw"] + g] = u0[:, d0["intercept"] + g], u0[:, d0["sigma_raw"] + g]
        if g < k:
            for c in range(1, Cc):
                u[:, slope_index(d1, Cc, c, g)] = u0[:, slope_index(d0, C0, c, g)]
    return dict(ds, X=np.ascontiguousarray(ds["X"][:, :Cc]), draws=u)


_SETS = {}


def draw_set(name):
    """ "covariate", "factor4", "columns8" and "columns16" at 1 000 draws; "long": "factor4" at 4 097 draws (its prefixes are the
    draw counts of the device test); "columns15": "columns16" cut down to its first 15 columns ((C + 1)^2 = 256, the workgroup's
    size). Built once."""
    if name not in _SETS:
        if name == "columns15":
            _SETS[name] = cut_columns(draw_set("columns16"), 15)
        else:
            _SETS[name] = wide_set("factor4", n=4097, seed=23) if name == "long" else wide_set(name)
    return _SETS[name]


def designed(widest=False):
    """dicts of name, set, g, s, r_eff, k_threshold, max_iters and `kinds`, as tests/loo_mm_cases.designed() gives them.
    widest: the cells of "columns8" and "columns16" instead (a list of their own: the cells of C = 3 and 4 stay the list they
    were, with the constants recorded for them)"""
    cs = []

    def add(name, set_, g, s, kinds, r_eff=1.0, k_threshold=0.7, max_iters=30):
        cs.append(dict(name=name, set=set_, g=g, s=s, kinds=kinds, r_eff=r_eff, k_threshold=k_threshold, max_iters=max_iters))

    if widest:
        add("columns8: one shift (d = 9)", "columns8", 0, 0, [1], k_threshold=0.5)
        add("columns8: one shift in gene 1", "columns8", 1, 10, [1])
        add("columns8: shift, then shift and scale", "columns8", 1, 4, [1, 2])
        add("columns8: shift and scale first at gene 1's outlier", "columns8", 1, 2, [2, 1, 2], k_threshold=0.5)
        add("columns8: r_eff = 0.4", "columns8", 0, 6, [1, 2, 2], r_eff=0.4)
        add("columns8: outlier in the unchecked gene", "columns8", 2, 1, [1])
        add("columns8: four steps in the unchecked gene", "columns8", 2, 1, [1, 1, 1, 2], k_threshold=0.1)
        add("columns8: excluded cell", "columns8", 1, 3, [])
        add("columns8: below the threshold", "columns8", 0, 7, [])
        add("columns8: stops at max_iters", "columns8", 1, 6, [1, 2], max_iters=2)
        add("columns16: one shift (d = 17)", "columns16", 0, 1, [1])
        add("columns16: one shift at a level that occurs once", "columns16", 0, 7, [1])
        add("columns16: shift, shift and scale, shift", "columns16", 0, 15, [1, 2, 1])
        add("columns16: shift, then two shifts and scales in gene 1", "columns16", 1, 7, [1, 2, 2])
        add("columns16: shift and scale alone", "columns16", 0, 8, [2])
        add("columns16: r_eff = 0.4", "columns16", 1, 9, [2, 1], r_eff=0.4, k_threshold=0.5)
        add("columns16: outlier in the unchecked gene", "columns16", 2, 1, [1])
        add("columns16: three steps in the unchecked gene", "columns16", 2, 1, [1, 1, 2], k_threshold=0.1)
        add("columns16: excluded cell", "columns16", 1, 3, [])
        add("columns16: below the threshold", "columns16", 0, 3, [])
        add("columns16: stops at max_iters", "columns16", 1, 2, [1, 1], max_iters=2)
        add("columns16: stops at max_iters after a scale", "columns16", 0, 14, [1, 1, 2], max_iters=3)
        return cs
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
