"""An independent restatement of gene-local moment matching with the covariance step (ppcseq_amd/csrc/ppcx_loo_mm_cov.h) with
numpy and scipy: the affine state as a matrix product, np.cov-style centred sums, np.linalg.cholesky for the two factors and a
dense solve for L_w L^-1; for the split np.linalg.inv and np.linalg.slogdet of the FINAL transform -- deliberately not the
inverse accumulated along the accepted steps, which is the header's definition. The cells' log-likelihood, the priors and the
PSIS are those of tests/loo_mm_restate.py. Written from Paananen, Piironen, Buerkner, Vehtari (2021) and loo's shift_and_cov /
loo_moment_match_split as the header's comment states them for one gene; nothing here is shared with the header. Not run
against R. It also holds the loader of the CPU build of the header (tests/loo_mm_cov_twin) and the runner of that build's
stand-alone program under the host sanitizers:

    python -m tests.loo_mm_cov_restate --sanitize

(and, with --factor4, the figures of the factor4 cell that DESIGN 8.15 records).

Shared by tests/test_loo_mm_cov_host.py (CPU) and tests/test_gpu_loo_mm_cov.py (device). A gene is the dict of
tests/loo_mm_restate.py.

MEASURED: the largest error of the CPU build against this restatement over tests/loo_mm_cov_cases.designed(), split both ways,
in elpd_loo, khat, khat_split, elpd_loo_matched, transform and shift, in units of max(1, |ref|)
(test_twin_matches_restatement prints it: 4.33e-11) and the two draw-count cells of test_draw_count_cells_qualify (5.75e-11 at
n = 4096). GPU_MEASURED: that of the device against the CPU build over the designed cells
(3.99e-11) and the draw counts (3.0e-11 at n = 4097) of tests/test_gpu_loo_mm_cov.py, which prints them. The bound of either comparison is ten times the measured
value and never above BOUND."""
import ctypes as C
import sys

import numpy as np

from tests import host_build
from tests import loo_mm_restate as R

HEAD = R.HEAD + ("cov_iterations", "elpd_loo_matched", "khat_split")
BOUND = 1e-9
MEASURED = 5.8e-11                                   # 4.33e-11 on the designed cells, 5.75e-11 on the draw-count cells (n = 4096)
GPU_MEASURED = 4.0e-11                               # 3.99e-11 on the designed cells, 3.0e-11 on the draw counts (n = 4097)
PIVOT = 1e-12                                        # the header's kLooMmCovPivot, stated again


def fields(Cc):
    return len(HEAD) + (Cc + 1) * (Cc + 1) + (Cc + 1)


# ---- the statistic

def coords(gene):
    nc = gene["T"].shape[0]
    return np.array([c for c in range(nc) if R.is_coord(gene, c)])


def transformed(gene, M, b):
    """t [C + 1, n] = M theta + b; a row that is no coordinate of the gene is the table's"""
    T = np.asarray(gene["T"], np.float64)
    ix = coords(gene)
    t = T.copy()
    t[ix] = np.asarray(M, np.float64)[np.ix_(ix, ix)] @ T[ix] + np.asarray(b, np.float64)[ix, None]
    return t


def local_density(gene, M, b):
    """(q [n], ll [S, n]) at the points M theta + b: loo_mm_restate.local_density's terms"""
    from scipy.stats import norm
    t = transformed(gene, M, b)
    Cc = gene["X"].shape[1]
    h = R.hyper(gene["U"], gene["lambda_mu_mu"])
    ll = R.cell_log_lik(gene, t)
    q = ll[~np.asarray(gene["excl"], bool)].sum(axis=0)
    q = q + R.log_skew_normal_kernel(t[0], h["xi"], h["om"], h["skew"])
    q = q + norm.logpdf(t[Cc], h["slope"] * t[0] + h["icpt"], h["ss"]) + np.log(h["ss"])
    if gene["checked"]:
        for c in range(1, Cc):
            q = q + (-np.abs(t[c]) if c == 1 else norm.logpdf(t[c], 0.0, 2.5))
    return q, ll


def moments(gene, M, b, w):
    """m, mw [d], Sigma, Sigma_w [d, d] (None where they are not defined) of the gene's coordinates of the current draws"""
    t = transformed(gene, M, b)[coords(gene)]
    d, n = t.shape
    m, mw = t.mean(axis=1), (w * t).sum(axis=1)
    den = 1.0 - np.sum(w * w)
    if n <= d or not (np.isfinite(den) and den > 0):
        return m, mw, None, None
    c0, cw = t - m[:, None], t - mw[:, None]
    return m, mw, c0 @ c0.T / (n - 1), (w * cw) @ cw.T / den


def cov_candidate(gene, M, b, w):
    """candidate 3 as (M', b'), or None where it is invalid"""
    ix = coords(gene)
    m, mw, sig, sig_w = moments(gene, M, b, w)
    if sig is None or not (np.all(np.isfinite(sig)) and np.all(np.isfinite(sig_w))):
        return None
    try:
        L, Lw = np.linalg.cholesky(sig), np.linalg.cholesky(sig_w)
    except np.linalg.LinAlgError:
        return None
    for A, F in ((sig, L), (sig_w, Lw)):              # a pivot at rounding noise of its diagonal entry: singular
        piv = np.diag(F) ** 2
        if not (np.all(np.isfinite(piv)) and np.all(piv > PIVOT * np.diag(A))):
            return None
    Tm = np.linalg.solve(L.T, Lw.T).T
    M2, b2 = np.array(M, np.float64), np.array(b, np.float64)
    M2[np.ix_(ix, ix)] = Tm @ M[np.ix_(ix, ix)]
    b2[ix] = Tm @ (b[ix] - m) + mw
    return M2, b2


def split_weights(gene, s, M, b, r_eff):
    """steps 2 - 6 of the split with the inverse and the determinant of the final map: (log weights [n], khat_split, the cell's
    log-likelihood at the proposal points [n])"""
    nc, n = gene["T"].shape
    h = n // 2
    ix = coords(gene)
    Minv, binv = np.eye(nc), np.zeros(nc)
    Minv[np.ix_(ix, ix)] = np.linalg.inv(M[np.ix_(ix, ix)])
    binv[ix] = -Minv[np.ix_(ix, ix)] @ b[ix]
    sign, log_j = np.linalg.slogdet(M[np.ix_(ix, ix)])
    assert sign > 0
    q_t, ll_t = local_density(gene, M, b)
    q_0, ll_0 = local_density(gene, np.eye(nc), np.zeros(nc))
    q_i, _ = local_density(gene, Minv, binv)
    first = np.arange(n) < h
    qx, llx = np.where(first, q_t, q_0), np.where(first, ll_t[s], ll_0[s])
    dd = np.where(first, q_0, q_i) - log_j
    with np.errstate(invalid="ignore"):
        r = qx - llx - np.logaddexp(qx, dd)
    lw, k = R.psis(np.where(np.isfinite(r), r, -np.inf), r_eff)
    return lw, k, llx


def point(gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, split=False, perturb=None, cov=True):
    """dict of the cell's fields, `transform` [C + 1, C + 1], `shift` [C + 1] and `kinds` (the accepted candidates in order).
    perturb: as loo_mm_restate.point. cov=False: the third candidate switched off (loo_mm_restate.point's path)."""
    L = R.L
    Cc = gene["X"].shape[1]
    nc = Cc + 1
    n = gene["T"].shape[1]
    M, b = np.eye(nc), np.zeros(nc)
    use = np.array([R.is_coord(gene, c) for c in range(nc)])
    excluded = bool(gene["excl"][s])
    jig = (lambda r: r) if perturb is None else (lambda r: r * (1.0 + perturb[1] * perturb[0].uniform(-1.0, 1.0, r.size)))
    Q0, ll_all = local_density(gene, M, b)
    ll = ll_all[s]
    plain = L.loo_point(ll, r_eff, excluded)
    out = dict(zip(R.HEAD, plain + (plain[3], 0)), cov_iterations=0, elpd_loo_matched=plain[0], khat_split=np.nan, transform=M.copy(),
               shift=b.copy(), kinds=[])
    if excluded or max_iters <= 0 or not (plain[3] > k_threshold) or not (ll != np.inf).any():
        return out
    lpd = plain[0] + plain[1]
    r = jig(-ll)
    r[np.isinf(ll) & (ll > 0)] = -np.inf
    lw, k = R.psis(r, r_eff)
    if perturb is not None and not (k > k_threshold):
        out["kinds"] = None                           # the perturbation moved the cell across the threshold
        return out
    while k > k_threshold and len(out["kinds"]) < max_iters:
        w = np.exp(lw - L.logsumexp(lw))
        t = transformed(gene, M, b)
        m, v = t.mean(axis=1), t.var(axis=1, ddof=1) if n > 1 else np.full(nc, np.nan)
        mw = (w * t).sum(axis=1)
        vw = (w * t * t).sum(axis=1) - mw * mw
        with np.errstate(invalid="ignore", divide="ignore"):
            sc = np.where(use, np.sqrt(vw / v), 1.0)

        def cands():
            yield 1, M.copy(), np.where(use, b + (mw - m), b)
            if np.all(np.isfinite(sc) & (sc > 0)):
                yield 2, sc[:, None] * M, np.where(use, sc * (b - m) + mw, b)
            if cov:
                c3 = cov_candidate(gene, M, b, w)
                if c3 is not None:
                    yield (3,) + c3

        for kind, M2, b2 in cands():
            q, ll2 = local_density(gene, M2, b2)
            with np.errstate(invalid="ignore"):
                r = q - Q0 - ll2[s]
            r = jig(np.where(np.isfinite(r), r, -np.inf))
            lw2, k2 = R.psis(r, r_eff)
            if k2 < k:
                M, b, lw, k = M2, b2, lw2, k2
                out["kinds"].append(kind)
                break
        else:
            break
    if not out["kinds"]:
        return out
    part = lw != -np.inf
    llf = R.cell_log_lik(gene, transformed(gene, M, b))[s]
    elpd = L.logsumexp(lw[part] + llf[part]) - L.logsumexp(lw[part])
    out.update(elpd_loo=elpd, p_loo=lpd - elpd, looic=-2.0 * elpd, khat=k, iterations=len(out["kinds"]),
               cov_iterations=out["kinds"].count(3), elpd_loo_matched=elpd, transform=M, shift=b)
    if split:
        lw, ks, llx = split_weights(gene, s, M, b, r_eff)
        part = lw != -np.inf
        if not part.any():
            out.update(elpd_loo=np.nan, p_loo=np.nan, looic=np.nan)
            return out
        es = L.logsumexp(lw[part] + llx[part]) - L.logsumexp(lw[part])
        out.update(elpd_loo=es, p_loo=lpd - es, looic=-2.0 * es, khat_split=ks)
    return out


def qualifies(gene, s, ref, r_eff=1.0, k_threshold=0.7, max_iters=30, runs=10, rel=1e-9, seed=5):
    """whether the integer decisions of a case (the accepted candidate kinds, hence both iteration counts) are the same under
    `runs` perturbations of every ratio by `rel` relative"""
    rng = np.random.default_rng(seed)
    return all(point(gene, s, r_eff, k_threshold, max_iters, perturb=(rng, rel))["kinds"] == ref["kinds"] for _ in range(runs))


def as_row(ref):
    """point()'s dict as the [9 + (C + 1)^2 + (C + 1)] record of the header"""
    return np.concatenate([[ref[k] for k in HEAD], np.asarray(ref["transform"]).ravel(), ref["shift"]]).astype(np.float64)


def row_dict(row, Cc):
    nc = Cc + 1
    out = dict(zip(HEAD, row[:len(HEAD)]))
    out["transform"] = np.asarray(row[len(HEAD):len(HEAD) + nc * nc]).reshape(nc, nc)
    out["shift"] = np.asarray(row[len(HEAD) + nc * nc:])
    return out


REALS = (0, 3, 7, 8)                                  # elpd_loo, khat, elpd_loo_matched, khat_split
INTS = (5, 6)


def _err(g, r):
    g, r = float(g), float(r)
    if not np.isfinite(r):
        return 0.0 if (np.isnan(r) and np.isnan(g)) or g == r else np.inf
    return abs(g - r) / max(1.0, abs(r))


def errors(got, ref_row):
    """the largest error of elpd_loo, khat, khat_split, elpd_loo_matched, transform and shift in units of max(1, |ref|); values
    that are not finite must be equal"""
    return max(_err(got[i], ref_row[i]) for i in list(REALS) + list(range(len(HEAD), len(ref_row))))


# ---- the CPU build of the header

def host_lib():
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    gene = [dp, dp, C.c_long, C.c_int, C.c_int, C.c_int, ip, dp, dp, C.c_double]
    return host_build.host_lib("loo_mm_cov_twin", {
        "loo_mm_cov_twin_cell": (gene + [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, dp, ip, dp], C.c_int)})


def host_cell(h, gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, split=False):
    """(the cell's record [9 + (C + 1)^2 + (C + 1)], the accepted kinds, dict(Minv, binv, logJ)) of the CPU build"""
    keep, args = R._gene_args(gene)
    nc = gene["X"].shape[1] + 1
    out = np.zeros(fields(nc - 1))
    kinds = np.zeros(max(1, int(max_iters)), np.int32)
    inv = np.zeros(nc * nc + nc + 1)
    nk = h.loo_mm_cov_twin_cell(*args, int(s), float(r_eff), float(k_threshold), int(max_iters), int(bool(split)), R._dp(out),
                                kinds.ctypes.data_as(C.POINTER(C.c_int)), R._dp(inv))
    return out, kinds[:nk].tolist(), dict(Minv=inv[:nc * nc].reshape(nc, nc), binv=inv[nc * nc:nc * nc + nc], logJ=inv[-1])


def sanitize():
    """the twin's stand-alone program under the host sanitizers (python -m tests.host_build --sanitize loo_mm_cov_twin); its exit status"""
    return host_build.sanitize(["loo_mm_cov_twin"])


def factor4():
    """the factor4 cell of DESIGN 8.15 (set factor4, gene 0, sample 5) under this restatement: plain PSIS, the matching without
    and with the covariance candidate"""
    from tests import loo_mm_cases, wide_design_cases
    gene = loo_mm_cases.gene_of(wide_design_cases.draw_set("factor4"), 0)
    plain = point(gene, 5, max_iters=0)
    print("plain PSIS: khat", plain["khat"], "elpd_loo", plain["elpd_loo"], flush=True)
    for cov in (False, True):
        p = point(gene, 5, cov=cov)
        print("covariance candidate", cov, "kinds", p["kinds"], "khat", p["khat"], "elpd_loo", p["elpd_loo"], flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["--factor4"]:
        factor4()
        sys.exit(0)
    if sys.argv[1:] != ["--sanitize"]:
        sys.exit("usage: python -m tests.loo_mm_cov_restate --sanitize | --factor4")
    sys.exit(sanitize())
