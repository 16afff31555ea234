"""An independent restatement of the gene-local moment matching of PSIS-LOO cells (ppcseq_amd/csrc/ppcx_loo_mm.h) with numpy and
scipy (nbinom.logpmf for the cells, norm.logpdf and erfc for the priors, the skew-normal against skewnorm.logpdf in
tests/test_loo_mm_host.py), the PSIS of tests/loo_restate.psis_log_weights, and the CPU build of the header (tests/loo_mm_host).
Written from the paper's algorithm (Paananen, Piironen, Buerkner, Vehtari 2021) as the header's comment states it for one gene;
nothing here is shared with the code under test. Shared by tests/test_loo_mm_host.py (CPU) and tests/test_gpu_loo_mm.py (device).

A gene is a dict: T [C + 1, n] (rows intercept, slopes, sigma_raw of the draws), U [6, n] (the draws' unconstrained
hyper-parameters lambda_mu, log lambda_sigma, lambda_skew, log -sigma_slope, sigma_intercept, log sigma_sigma), y [S], excl [S],
expo [S], X [S, C], checked, lambda_mu_mu.

MEASURED: the largest error of the CPU build against this restatement in khat, elpd_loo, scale and shift over
tests/loo_mm_cases.designed(), in units of max(1, |ref|) (test_header_matches_restatement prints it); GPU_MEASURED: that of the
device against the CPU build over the designed cells (8.8e-12) and the draw counts of tests/test_gpu_loo_mm.py (1.9e-11 at
n = 64), which prints both. The bound of either comparison is ten times the measured
value and never above BOUND."""
import ctypes as C

import numpy as np

from tests import host_build
from tests import loo_restate as L

HEAD = ("elpd_loo", "p_loo", "looic", "khat", "khat_before", "iterations")
BOUND = 1e-9
MEASURED = 1.8e-11
GPU_MEASURED = 1.9e-11


def fields(Cc):
    return len(HEAD) + 2 * (Cc + 1)


# ---- the statistic

def hyper(U, lambda_mu_mu):
    """the constrained hyper-parameters of the draws: xi, lambda_sigma, lambda_skew, sigma_slope, sigma_intercept, sigma_sigma"""
    U = np.asarray(U, np.float64)
    return dict(xi=U[0] + 2.0 * lambda_mu_mu, om=np.exp(U[1]), skew=U[2], slope=-np.exp(U[3]), icpt=U[4], ss=np.exp(U[5]))


def transformed(gene, A, B):
    return np.asarray(A, np.float64)[:, None] * gene["T"] + np.asarray(B, np.float64)[:, None]


def cell_log_lik(gene, t):
    """[S, n] log-likelihood of every cell of the gene at the coordinates t [C + 1, n]"""
    Cc = gene["X"].shape[1]
    eta = gene["expo"][:, None] + gene["X"] @ t[:Cc]
    return np.stack([L.log_lik(int(gene["y"][s]), eta[s], t[Cc]) for s in range(eta.shape[0])])


def log_skew_normal_kernel(x, xi, om, skew):
    """the skew-normal log density up to the terms without x: -z^2 / 2 + log erfc(-skew z / sqrt 2) (-Inf where erfc underflows)"""
    from scipy.special import erfc
    z = (x - xi) / om
    with np.errstate(divide="ignore"):
        return -0.5 * z * z + np.log(erfc(-skew * z / np.sqrt(2.0)))


def local_density(gene, A, B):
    """(q [n], ll [S, n]) under the state (A, B): the log-likelihoods of the cells the model does not exclude plus the gene's
    prior terms, up to terms that do not depend on the gene's coordinates"""
    from scipy.stats import norm
    t = transformed(gene, A, B)
    Cc = gene["X"].shape[1]
    h = hyper(gene["U"], gene["lambda_mu_mu"])
    ll = cell_log_lik(gene, t)
    q = ll[~np.asarray(gene["excl"], bool)].sum(axis=0)
    q = q + log_skew_normal_kernel(t[0], h["xi"], h["om"], h["skew"])
    q = q + norm.logpdf(t[Cc], h["slope"] * t[0] + h["icpt"], h["ss"]) + np.log(h["ss"])
    if gene["checked"]:
        for c in range(1, Cc):
            q = q + (-np.abs(t[c]) if c == 1 else norm.logpdf(t[c], 0.0, 2.5))
    return q, ll


def is_coord(gene, c):
    Cc = gene["X"].shape[1]
    return c == 0 or c == Cc or bool(gene["checked"])


def psis(r, r_eff):
    """(log weights [n] in draw order, -Inf for a draw that takes no part; k-hat) of the ratios r (-Inf: no part)"""
    part = r != -np.inf
    lw = np.full(r.size, -np.inf)
    if not part.any():
        return lw, np.inf
    lw[part], kh = L.psis_log_weights(r[part], r_eff)
    return lw, kh


def point(gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, perturb=None):
    """dict of the cell's fields, `scale` and `shift` [C + 1] and `kinds` (the accepted candidates in order). perturb: None, or
    (rng, rel): every ratio is multiplied by 1 + rel u, u uniform in [-1, 1] (the qualification of a designed case)."""
    Cc = gene["X"].shape[1]
    nc = Cc + 1
    n = gene["T"].shape[1]
    A, B = np.ones(nc), np.zeros(nc)
    excluded = bool(gene["excl"][s])
    jig = (lambda r: r) if perturb is None else (lambda r: r * (1.0 + perturb[1] * perturb[0].uniform(-1.0, 1.0, r.size)))
    Q0, ll_all = local_density(gene, A, B)
    ll = ll_all[s]
    plain = L.loo_point(ll, r_eff, excluded)
    out = dict(zip(HEAD, plain + (plain[3], 0)), scale=A.copy(), shift=B.copy(), kinds=[])
    if excluded or max_iters <= 0 or not (plain[3] > k_threshold) or not (ll != np.inf).any():
        return out
    lpd = plain[0] + plain[1]
    r = jig(-ll)
    r[np.isinf(ll) & (ll > 0)] = -np.inf
    lw, k = psis(r, r_eff)
    if perturb is not None and not (k > k_threshold):
        out["kinds"] = None                           # the perturbation moved the cell across the threshold
        return out
    while k > k_threshold and len(out["kinds"]) < max_iters:
        w = np.exp(lw - L.logsumexp(lw))
        t = transformed(gene, A, B)
        m, v = t.mean(axis=1), t.var(axis=1, ddof=1) if n > 1 else np.full(nc, np.nan)
        mw = (w * t).sum(axis=1)
        vw = (w * t * t).sum(axis=1) - mw * mw
        use = np.array([is_coord(gene, c) for c in range(nc)])
        with np.errstate(invalid="ignore", divide="ignore"):
            sc = np.where(use, np.sqrt(vw / v), 1.0)
        cands = [(1, A.copy(), np.where(use, B + (mw - m), B))]
        if np.all(np.isfinite(sc) & (sc > 0)):
            cands.append((2, sc * A, np.where(use, sc * (B - m) + mw, B)))
        for kind, A2, B2 in cands:
            q, ll2 = local_density(gene, A2, B2)
            with np.errstate(invalid="ignore"):
                r = q - Q0 - ll2[s]
            r = jig(np.where(np.isfinite(r), r, -np.inf))
            lw2, k2 = psis(r, r_eff)
            if k2 < k:
                A, B, lw, k = A2, B2, lw2, k2
                out["kinds"].append(kind)
                break
        else:
            break
    if out["kinds"]:
        part = lw != -np.inf
        llf = cell_log_lik(gene, transformed(gene, A, B))[s]
        elpd = L.logsumexp(lw[part] + llf[part]) - L.logsumexp(lw[part])
        out.update(elpd_loo=elpd, p_loo=lpd - elpd, looic=-2.0 * elpd, khat=k, iterations=len(out["kinds"]), scale=A, shift=B)
    return out


def qualifies(gene, s, ref, r_eff=1.0, k_threshold=0.7, max_iters=30, runs=10, rel=1e-9, seed=5):
    """whether the integer decisions of a case (the accepted candidate kinds, hence the iteration count) are the same under `runs`
    perturbations of every ratio by `rel` relative"""
    rng = np.random.default_rng(seed)
    return all(point(gene, s, r_eff, k_threshold, max_iters, perturb=(rng, rel))["kinds"] == ref["kinds"] for _ in range(runs))


def as_row(ref):
    """point()'s dict as the [6 + 2 (C + 1)] record of the header"""
    return np.concatenate([[ref[k] for k in HEAD], ref["scale"], ref["shift"]]).astype(np.float64)


def errors(got, ref_row):
    """the largest error of khat, elpd_loo, scale and shift in units of max(1, |ref|); values that are not finite must be equal"""
    worst = 0.0
    for i in [0, 3] + list(range(len(HEAD), len(ref_row))):
        g, r = float(got[i]), float(ref_row[i])
        if not np.isfinite(r):
            worst = max(worst, 0.0 if (np.isnan(r) and np.isnan(g)) or g == r else np.inf)
        else:
            worst = max(worst, abs(g - r) / max(1.0, abs(r)))
    return worst


# ---- the CPU build of the header

def host_lib():
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    gene = [dp, dp, C.c_long, C.c_int, C.c_int, C.c_int, ip, dp, dp, C.c_double]
    return host_build.host_lib("loo_mm", {
        "loo_mm_host_cell": (gene + [C.c_int, C.c_double, C.c_double, C.c_int, dp, ip], C.c_int),
        "loo_mm_host_density": (gene + [C.c_int, dp, dp, dp, dp], None),
        "loo_mm_host_loo_cell": ([dp, C.c_long, C.c_double, C.c_int, dp], None)})


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _gene_args(gene):
    T = np.ascontiguousarray(gene["T"], np.float64)
    U = np.ascontiguousarray(gene["U"], np.float64)
    y = np.asarray(gene["y"], np.int64)
    yenc = np.ascontiguousarray(np.where(np.asarray(gene["excl"], bool), -y - 1, y), np.int32)
    expo = np.ascontiguousarray(gene["expo"], np.float64)
    X = np.ascontiguousarray(np.asarray(gene["X"], np.float64).T)          # [C][S]
    keep = (T, U, yenc, expo, X)
    return keep, [_dp(T), _dp(U), T.shape[1], X.shape[0], X.shape[1], int(bool(gene["checked"])),
                  yenc.ctypes.data_as(C.POINTER(C.c_int)), _dp(expo), _dp(X), float(gene["lambda_mu_mu"])]


def host_cell(h, gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30):
    """(the cell's record [6 + 2 (C + 1)], the accepted kinds) of the CPU build"""
    keep, args = _gene_args(gene)
    out = np.zeros(fields(gene["X"].shape[1]))
    kinds = np.zeros(max(1, int(max_iters)), np.int32)
    nk = h.loo_mm_host_cell(*args, int(s), float(r_eff), float(k_threshold), int(max_iters), _dp(out),
                            kinds.ctypes.data_as(C.POINTER(C.c_int)))
    return out, kinds[:nk].tolist()


def host_density(h, gene, s, A, B):
    """(q [n], the log-likelihood of cell s [n]) of the CPU build under the state (A, B)"""
    keep, args = _gene_args(gene)
    n = gene["T"].shape[1]
    A, B = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(B, np.float64)
    q, ll = np.zeros(n), np.zeros(n)
    h.loo_mm_host_density(*args, int(s), _dp(A), _dp(B), _dp(q), _dp(ll))
    return q, ll


def host_loo_cell(h, ll, r_eff=1.0, excluded=False):
    ll = np.ascontiguousarray(ll, np.float64)
    out = np.zeros(4)
    h.loo_mm_host_loo_cell(_dp(ll), ll.size, float(r_eff), int(excluded), _dp(out))
    return out
