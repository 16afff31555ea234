"""Designed draws shared by tests/test_loo_mm_host.py (CPU) and tests/test_gpu_loo_mm.py (device) for the gene-local moment
matching of PSIS-LOO cells: a tiny model (S = 4 samples, C = 2 design columns, one checked gene with d = 3 coordinates, one
unchecked gene with d = 2, one excluded cell in the checked gene's row) whose genes' draws come from their exact posterior given
the hyper-parameters, tabulated on a grid; and the one-gene truth case (C = 1, S = 6) whose held-out density is known by
quadrature on the same grid.

A draw set is a dict: counts [G, S], X [S, C], expo [S], K, excl (flat cell ids), lambda_mu_mu, draws [n, D] in the model's
unconstrained order. gene_of() cuts one gene out of it in the form tests/loo_mm_restate.py takes, for any C (the draw sets with
more than one slope are tests/wide_design_cases.py's)."""
import numpy as np

from tests import loo_restate as L

LAMBDA_MU_MU = 5.612671
# xi = 6.5, lambda_sigma 1.8, lambda_skew -1, sigma_slope -0.3, sigma_intercept 0, sigma_sigma 0.4, unconstrained
HYPER = np.array([6.5 - 2.0 * LAMBDA_MU_MU, np.log(1.8), -1.0, np.log(0.3), 0.0, np.log(0.4)])


def dims(G, Cc, K):
    """offsets of the unconstrained vector (the model's declaration order)"""
    off_i, off_a1 = 3, 3 + G
    off_a2 = off_a1 + K
    off_sg = off_a2 + max(Cc - 2, 0) * K
    return dict(D=off_sg + G + 3, intercept=off_i, alpha1=off_a1, alpha2=off_a2, sigma_raw=off_sg, tail=off_sg + G)


def slope_index(d, Cc, c, g):
    """where slope c >= 1 of checked gene g lies in the unconstrained vector: alpha1 holds the K first slopes gene by gene, alpha2
    the C - 2 further slopes of gene 0, then those of gene 1, ... (written out here, not taken from the header)"""
    return d["alpha1"] + g if c == 1 else d["alpha2"] + (c - 2) + (Cc - 2) * g


def gene_of(ds, g):
    """gene g of a draw set as tests/loo_mm_restate.py takes it. General in C: row c of a checked gene is its slope c for every
    1 <= c < C (tests/wide_design_cases.py has C = 3 and 4); at C <= 2 the rows are what they were, bit for bit."""
    G, S = ds["counts"].shape
    Cc = ds["X"].shape[1]
    d = dims(G, Cc, ds["K"])
    u = ds["draws"]
    n = u.shape[0]
    T = np.zeros((Cc + 1, n))
    T[0] = u[:, d["intercept"] + g]
    if g < ds["K"] and Cc >= 2:
        for c in range(1, Cc):
            T[c] = u[:, slope_index(d, Cc, c, g)]
    T[Cc] = u[:, d["sigma_raw"] + g]
    U = np.stack([u[:, 0], u[:, 1], u[:, 2], u[:, d["tail"]], u[:, d["tail"] + 1], u[:, d["tail"] + 2]])
    excl = np.zeros(G * S, bool)
    excl[np.asarray(ds["excl"], np.int64)] = True
    return dict(T=T, U=U, y=ds["counts"][g], excl=excl.reshape(G, S)[g], expo=ds["expo"], X=ds["X"],
                checked=bool(g < ds["K"] and Cc >= 2), lambda_mu_mu=ds["lambda_mu_mu"])


def _grid_log_post(y, excl, expo, X, checked, axes):
    """the gene's log posterior given HYPER on the product grid of `axes` (intercept, [slope,] sigma_raw), up to a constant"""
    from tests import loo_mm_restate as R
    mesh = np.meshgrid(*axes, indexing="ij")
    shape = mesh[0].shape
    Cc = X.shape[1]
    T = np.zeros((Cc + 1, mesh[0].size))
    T[0] = mesh[0].ravel()
    if checked:
        T[1] = mesh[1].ravel()
    T[Cc] = mesh[-1].ravel()
    gene = dict(T=T, U=np.repeat(HYPER[:, None], T.shape[1], axis=1), y=y, excl=excl, expo=expo, X=X, checked=checked,
                lambda_mu_mu=LAMBDA_MU_MU)
    q, ll = R.local_density(gene, np.ones(Cc + 1), np.zeros(Cc + 1))
    return q.reshape(shape), ll.reshape((len(y),) + shape)


def grid_draws(rng, n, y, excl, expo, X, checked, axes):
    """n draws of the gene's coordinates from its posterior given HYPER tabulated on the grid, with uniform jitter within a
    grid step: [n, len(axes)]"""
    lp, _ = _grid_log_post(y, excl, expo, X, checked, axes)
    p = np.exp(lp - lp.max()).ravel()
    ix = rng.choice(p.size, size=n, p=p / p.sum())
    sub = np.unravel_index(ix, lp.shape)
    return np.stack([ax[k] + rng.uniform(-0.5, 0.5, n) * (ax[1] - ax[0]) for ax, k in zip(axes, sub)], axis=1)


X2 = np.array([[1.0, 0.0], [1.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
EXPO2 = np.array([0.0, 0.1, -0.1, 0.05])


def tiny_set(seed, n, counts, excl_cells=((0, 2),), hyper_jitter=0.02):
    """a draw set of the tiny model: gene 0 checked (intercept, slope, sigma_raw), gene 1 not (intercept, sigma_raw)"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int32)
    G, S = counts.shape
    d = dims(G, 2, 1)
    excl = np.zeros((G, S), bool)
    for g, s in excl_cells:
        excl[g, s] = True
    u = np.zeros((n, d["D"]))
    h = HYPER[None, :] + rng.normal(0.0, hyper_jitter, (n, 6))
    u[:, 0:3], u[:, d["tail"]:d["tail"] + 3] = h[:, :3], h[:, 3:]
    lo = np.log(np.maximum(counts, 1))
    t0 = grid_draws(rng, n, counts[0], excl[0], EXPO2, X2, True,
                    (np.linspace(lo[0].min() - 2.0, lo[0].max() + 1.0, 90), np.linspace(-3.0, 3.0, 90), np.linspace(-5.0, 2.0, 90)))
    t1 = grid_draws(rng, n, counts[1], excl[1], EXPO2, X2, False,
                    (np.linspace(lo[1].min() - 2.0, lo[1].max() + 1.0, 400), np.linspace(-6.0, 2.5, 400)))
    u[:, d["intercept"]], u[:, d["alpha1"]], u[:, d["sigma_raw"]] = t0[:, 0], t0[:, 1], t0[:, 2]
    u[:, d["intercept"] + 1], u[:, d["sigma_raw"] + 1] = t1[:, 0], t1[:, 1]
    return dict(counts=counts, X=X2, expo=EXPO2, K=1, excl=np.flatnonzero(excl.ravel()).astype(np.int32), lambda_mu_mu=LAMBDA_MU_MU,
                draws=u)


# ---- the truth case: one gene, C = 1, S = 6, hyper-parameters fixed over the draws
TRUTH_COUNTS = np.array([[120, 180, 95, 160, 140, 900]], np.int32)
TRUTH_GRID = (np.linspace(2.5, 9.5, 900), np.linspace(-5.5, 3.0, 900))
TRUTH_CELL = 5


def truth_elpd():
    """the held-out log predictive density of the last cell by quadrature on TRUTH_GRID: log E[p(y_5 | theta)] under the
    posterior of the other five cells"""
    y = TRUTH_COUNTS[0]
    excl = np.zeros(6, bool)
    excl[TRUTH_CELL] = True
    lp, ll = _grid_log_post(y, excl, np.zeros(6), np.ones((6, 1)), False, TRUTH_GRID)
    return L.logsumexp((lp + ll[TRUTH_CELL]).ravel()) - L.logsumexp(lp.ravel())


def truth_set(seed, n):
    rng = np.random.default_rng(seed)
    d = dims(1, 1, 0)
    u = np.zeros((n, d["D"]))
    u[:, 0:3], u[:, d["tail"]:d["tail"] + 3] = HYPER[:3], HYPER[3:]
    t = grid_draws(rng, n, TRUTH_COUNTS[0], np.zeros(6, bool), np.zeros(6), np.ones((6, 1)), False, TRUTH_GRID)
    u[:, d["intercept"]], u[:, d["sigma_raw"]] = t[:, 0], t[:, 1]
    return dict(counts=TRUTH_COUNTS, X=np.ones((6, 1)), expo=np.zeros(6), K=0, excl=np.zeros(0, np.int32), lambda_mu_mu=LAMBDA_MU_MU,
                draws=u)


# ---- the designed cells
_SETS = {}


def draw_set(name):
    """the named draw sets of the designed cells (built once):
    "b": a moderate outlier in the checked gene; "c": strong outliers in both genes; "c, planted": "c" with twenty draws whose
    lambda_skew makes the skew-normal prior of gene 0 underflow (ten of them at every intercept in reach: log erfc = -Inf at the
    original draws already; ten on the way to it: log erfc = -326 there); "nan": "b" at 400 draws with a NaN sigma_raw of gene 1 at one draw"""
    if name not in _SETS:
        if name == "b":
            ds = tiny_set(11, 1000, [[120, 180, 95, 400], [300, 280, 330, 40]])
        elif name == "c":
            ds = tiny_set(11, 1000, [[20, 35, 25, 4000], [300, 2, 330, 310]])
        elif name == "c, planted":
            ds = dict(draw_set("c"))
            u = ds["draws"].copy()
            d = dims(2, 2, 1)
            z = (u[:, d["intercept"]] - 6.5) / 1.8                          # < 0: gene 0's intercepts lie below xi
            u[100:110, 2] = 60.0                                           # erfc(60 |z| / sqrt 2) = 0
            u[200:210, 2] = 18.0 * np.sqrt(2.0) / np.abs(z[200:210])       # erfc(18): finite, 1e-143, and clear of the band
            #                                                                (26.5 .. 27.3) in which erfc is subnormal
            ds["draws"] = u
        elif name == "nan":
            ds = tiny_set(12, 400, [[120, 180, 95, 400], [300, 280, 330, 40]])
            ds["draws"][7, dims(2, 2, 1)["sigma_raw"] + 1] = np.nan
        else:
            raise KeyError(name)
        _SETS[name] = ds
    return _SETS[name]


def designed():
    """dicts of name, set (draw_set's name), g, s, r_eff, k_threshold, max_iters and `kinds`: the accepted candidates the case was
    designed to show (tests/test_loo_mm_host.py holds the restatement to them)"""
    cs = []

    def add(name, set_, g, s, kinds, r_eff=1.0, k_threshold=0.7, max_iters=30):
        cs.append(dict(name=name, set=set_, g=g, s=s, kinds=kinds, r_eff=r_eff, k_threshold=k_threshold, max_iters=max_iters))

    add("smooth cell", "c", 1, 0, [])
    add("one shift fixes the outlier", "b", 0, 3, [1])
    add("shift refused, shift and scale accepted (d = 3)", "c", 0, 3, [1, 2, 1, 1, 1, 1])
    add("shift refused, shift and scale accepted (d = 2)", "c", 1, 0, [1, 2], k_threshold=0.2)
    add("neither candidate accepted", "b", 0, 0, [], k_threshold=0.2)
    add("stops at max_iters", "c", 0, 3, [1, 2], max_iters=2)
    add("max_iters = 0", "c", 0, 3, [], max_iters=0)
    add("densities that are not finite at some draws", "c, planted", 0, 3, None)
    add("r_eff = 0.4", "b", 0, 3, None, r_eff=0.4)
    add("excluded cell", "c", 0, 2, [])
    add("nan cell", "nan", 1, 1, [])
    add("outlier in the unchecked gene", "c", 1, 1, [1, 1])
    return cs


def long_set():
    """4 097 draws of the tiny model with outliers in both genes: its prefixes are the draw counts of the device test"""
    if "long" not in _SETS:
        _SETS["long"] = tiny_set(13, 4097, [[20, 35, 25, 4000], [300, 2, 330, 310]])
    return _SETS["long"]


def prefix(ds, n):
    out = dict(ds)
    out["draws"] = ds["draws"][:n]
    return out
