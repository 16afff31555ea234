"""Designed draws shared by tests/test_loo_mm_ap_host.py (CPU) and tests/test_gpu_loo_mm_ap.py (device) for the gene-local moment
matching of the PSIS-LOO cells of an ADVI fit: the tiny model of tests/loo_mm_cases.py (S = 4 samples, C = 2 design columns, one
checked gene with d = 3 coordinates, one unchecked gene with d = 2, one excluded cell in the checked gene's row) with the genes'
coordinates drawn from a mean-field Gaussian g -- independent normals with the marginal means and standard deviations of each
gene's posterior given the hyper-parameters, tabulated on loo_mm_cases' grids -- and jittered hyper-parameters; and the one-gene
truth case (C = 1, S = 6) whose held-out density is known by quadrature, under the same kind of proposal.

A draw set is loo_mm_cases' dict plus `a` [n]: the draws' log ratios log_p - log_g, here the sum of both genes' local densities
minus log g of the genes' coordinates (the hyper-parameters count as drawn from their posterior: they add nothing to either)."""
import numpy as np

from tests import loo_mm_cases as M
from tests import loo_mm_restate as R

_MOMENTS = {}


def grid_moments(y, excl, expo, X, checked, axes):
    """(means, standard deviations) of the marginals of the gene's posterior given M.HYPER tabulated on the product grid"""
    lp, _ = M._grid_log_post(y, excl, expo, X, checked, axes)
    p = np.exp(lp - lp.max())
    p /= p.sum()
    mean, sd = [], []
    for k, ax in enumerate(axes):
        marg = p.sum(axis=tuple(j for j in range(len(axes)) if j != k))
        mu = float(np.sum(marg * ax))
        mean.append(mu)
        sd.append(float(np.sqrt(np.sum(marg * (ax - mu) ** 2))))
    return np.array(mean), np.array(sd)


def _tiny_moments(counts, excl):
    key = (counts.tobytes(), excl.tobytes())
    if key not in _MOMENTS:
        lo = np.log(np.maximum(counts, 1))
        _MOMENTS[key] = (
            grid_moments(counts[0], excl[0], M.EXPO2, M.X2, True,
                         (np.linspace(lo[0].min() - 2.0, lo[0].max() + 1.0, 90), np.linspace(-3.0, 3.0, 90), np.linspace(-5.0, 2.0, 90))),
            grid_moments(counts[1], excl[1], M.EXPO2, M.X2, False,
                         (np.linspace(lo[1].min() - 2.0, lo[1].max() + 1.0, 400), np.linspace(-6.0, 2.5, 400))))
    return _MOMENTS[key]


def _log_normal(x, mean, sd):
    return -0.5 * ((x - mean) / sd) ** 2 - np.log(sd) - 0.5 * np.log(2.0 * np.pi)


def log_ratios(ds, log_g):
    """a = the sum of the genes' local densities at the draws minus log_g"""
    G = ds["counts"].shape[0]
    Cc = ds["X"].shape[1]
    q = sum(R.local_density(M.gene_of(ds, g), np.ones(Cc + 1), np.zeros(Cc + 1))[0] for g in range(G))
    return q - log_g


def tiny_ap_set(seed, n, counts, excl_cells=((0, 2),), hyper_jitter=0.02, widen=1.0):
    """a draw set of the tiny model under the mean-field proposal; widen: the factor on the proposal's standard deviations"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int32)
    G, S = counts.shape
    d = M.dims(G, 2, 1)
    excl = np.zeros((G, S), bool)
    for g, s in excl_cells:
        excl[g, s] = True
    (m0, s0), (m1, s1) = _tiny_moments(counts, excl)
    u = np.zeros((n, d["D"]))
    h = M.HYPER[None, :] + rng.normal(0.0, hyper_jitter, (n, 6))
    u[:, 0:3], u[:, d["tail"]:d["tail"] + 3] = h[:, :3], h[:, 3:]
    t0 = m0 + widen * s0 * rng.normal(size=(n, 3))
    t1 = m1 + widen * s1 * rng.normal(size=(n, 2))
    u[:, d["intercept"]], u[:, d["alpha1"]], u[:, d["sigma_raw"]] = t0[:, 0], t0[:, 1], t0[:, 2]
    u[:, d["intercept"] + 1], u[:, d["sigma_raw"] + 1] = t1[:, 0], t1[:, 1]
    ds = dict(counts=counts, X=M.X2, expo=M.EXPO2, K=1, excl=np.flatnonzero(excl.ravel()).astype(np.int32), lambda_mu_mu=M.LAMBDA_MU_MU,
              draws=u)
    ds["a"] = log_ratios(ds, _log_normal(t0, m0, widen * s0).sum(axis=1) + _log_normal(t1, m1, widen * s1).sum(axis=1))
    return ds


# ---- the designed cells
_SETS = {}


def draw_set(name):
    """the named draw sets of the designed cells (built once):
    "b": a moderate outlier in either gene, the overall k-hat of a near 0.3; "c": strong outliers in both genes, the overall k-hat
    near 0.6; "c, -inf": "c" with a = -Inf at ten draws (a log_p or log_g that is not finite); "c, planted": "c" with loo_mm_cases'
    twenty planted draws whose lambda_skew makes the skew-normal prior of gene 0 underflow (ten with log erfc = -Inf at the original
    draws already, so that a = -Inf there by its own formula; ten on the way to it: log erfc = -326); "nan": "b" at 400 draws with
    a NaN sigma_raw of gene 1 at one draw, where a = -Inf as a fit would have it; "a, nan": "b" at 400 draws with a NaN in a"""
    if name not in _SETS:
        if name == "b":
            ds = tiny_ap_set(11, 1000, [[120, 180, 95, 400], [300, 280, 330, 40]])
        elif name == "c":
            ds = tiny_ap_set(11, 1000, [[20, 35, 25, 4000], [300, 2, 330, 310]])
        elif name == "c, -inf":
            ds = dict(draw_set("c"))
            ds["a"] = ds["a"].copy()
            ds["a"][50:60] = -np.inf
        elif name == "c, planted":
            ds = dict(draw_set("c"))
            u = ds["draws"].copy()
            d = M.dims(2, 2, 1)
            z = (u[:, d["intercept"]] - 6.5) / 1.8                          # < 0: gene 0's intercepts lie below xi
            u[100:110, 2] = 60.0                                           # erfc(60 |z| / sqrt 2) = 0
            u[200:210, 2] = 18.0 * np.sqrt(2.0) / np.abs(z[200:210])       # erfc(18): finite, 1e-143
            log_g = log_ratios(ds, 0.0) - ds["a"]                          # the proposal's density does not read lambda_skew
            ds["draws"] = u
            with np.errstate(invalid="ignore"):
                a = log_ratios(ds, log_g)
            ds["a"] = np.where(np.isfinite(a), a, -np.inf)
        elif name in ("nan", "a, nan"):
            ds = tiny_ap_set(12, 400, [[120, 180, 95, 400], [300, 280, 330, 40]])
            if name == "nan":
                ds["draws"][7, M.dims(2, 2, 1)["sigma_raw"] + 1] = np.nan
                ds["a"][7] = -np.inf
            else:
                ds["a"][7] = np.nan
        else:
            raise KeyError(name)
        _SETS[name] = ds
    return _SETS[name]


def designed():
    """dicts of name, set (draw_set's name), g, s, k_threshold, max_iters and `kinds`: the accepted candidates the case was
    designed to show (tests/test_loo_mm_ap_host.py holds the restatement to them; None: not stated)"""
    cs = []

    def add(name, set_, g, s, kinds, k_threshold=0.7, max_iters=30):
        cs.append(dict(name=name, set=set_, g=g, s=s, kinds=kinds, k_threshold=k_threshold, max_iters=max_iters))

    add("smooth cell", "b", 0, 1, [])
    add("one shift fixes the outlier", "c", 0, 1, [1])
    add("shift refused, shift and scale accepted (d = 3)", "c", 0, 3, [1, 1, 1, 1, 2, 2], k_threshold=0.2)
    add("shift refused, shift and scale accepted (d = 2)", "b", 1, 0, [2, 2, 2, 1], k_threshold=0.2)
    add("neither candidate accepted", "b", 1, 1, [], k_threshold=0.2)
    add("stops at max_iters", "c", 0, 3, [1, 1], k_threshold=0.2, max_iters=2)
    add("max_iters = 0", "c", 0, 3, [], max_iters=0)
    add("excluded cell", "c", 0, 2, [])
    add("nan cell", "nan", 1, 1, [])
    add("nan in the log ratios", "a, nan", 0, 3, [])
    add("a = -Inf at some draws", "c, -inf", 0, 3, None)
    add("densities that are not finite at some draws", "c, planted", 0, 3, None)
    add("outlier in the unchecked gene", "c", 1, 1, [1, 1])
    add("threshold below the overall k-hat", "c", 1, 3, None, k_threshold=0.5)
    return cs


def long_set():
    """4 097 draws of the tiny model with outliers in both genes: its prefixes are the draw counts of the device test"""
    if "long" not in _SETS:
        _SETS["long"] = tiny_ap_set(13, 4097, [[20, 35, 25, 4000], [300, 2, 330, 310]])
    return _SETS["long"]


def prefix(ds, n):
    out = dict(ds)
    out["draws"], out["a"] = ds["draws"][:n], ds["a"][:n]
    return out


# ---- the truth case: loo_mm_cases' gene and grid; the proposal is the Gaussian with the grid posterior's marginal moments
TRUTH_SEEDS = (0, 1, 2, 3, 4, 5)
TRUTH_DRAWS = 1000


def truth_ap_set(seed, n=TRUTH_DRAWS):
    """intercepts drawn first, then sigma_raw, from default_rng(seed)"""
    if "truth" not in _MOMENTS:
        _MOMENTS["truth"] = grid_moments(M.TRUTH_COUNTS[0], np.zeros(6, bool), np.zeros(6), np.ones((6, 1)), False, M.TRUTH_GRID)
    mean, sd = _MOMENTS["truth"]
    rng = np.random.default_rng(seed)
    d = M.dims(1, 1, 0)
    u = np.zeros((n, d["D"]))
    u[:, 0:3], u[:, d["tail"]:d["tail"] + 3] = M.HYPER[:3], M.HYPER[3:]
    t = np.stack([rng.normal(mean[0], sd[0], n), rng.normal(mean[1], sd[1], n)], axis=1)
    u[:, d["intercept"]], u[:, d["sigma_raw"]] = t[:, 0], t[:, 1]
    ds = dict(counts=M.TRUTH_COUNTS, X=np.ones((6, 1)), expo=np.zeros(6), K=0, excl=np.zeros(0, np.int32), lambda_mu_mu=M.LAMBDA_MU_MU,
              draws=u)
    ds["a"] = log_ratios(ds, _log_normal(t, mean, sd).sum(axis=1))
    return ds
