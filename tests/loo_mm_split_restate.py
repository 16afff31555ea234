"""An independent restatement of the split transformation of gene-local moment matching (ppcseq_amd/csrc/ppcx_loo_mm_split.h,
steps 2 - 8) with numpy and scipy: the matching, the local density and the PSIS of tests/loo_mm_restate.py (point /
local_density / psis), np.logaddexp for the mixture, and the predictive of tests/loo_mm_exact_restate.py (nbinom.cdf / sf,
quantiles by bisection). Written from section 4 of Paananen, Piironen, Buerkner, Vehtari (2021) and loo's
loo_moment_match_split as the header's comment states them for one gene; nothing here is shared with the header. It also holds
the loader of the CPU build of the header (tests/loo_mm_split_twin) and the runner of that build's stand-alone program under
the host sanitizers:

    python -m tests.loo_mm_split_restate --sanitize

(and, with --fine-grid, the figures of the truth case on a 2500 x 2500 grid that DESIGN 8.13 records).

Shared by tests/test_loo_mm_split_host.py (CPU) and tests/test_gpu_loo_mm_split.py (device). A gene is the dict of
tests/loo_mm_restate.py.

MEASURED: the largest error of the CPU build against this restatement over tests/loo_mm_cases.designed() in elpd_loo,
khat_split, khat, scale and shift of the elpd form and mean, sd, p_le, p_ge, khat, khat_before, khat_split, scale and shift of
the predictive form, in units of max(1, |ref|), p_le / p_ge also relatively below 1e-3 (test_header_matches_restatement prints
it: 1.75e-11). GPU_MEASURED: that of the device against the CPU build over the designed cells (4.5e-11), the draw counts
(4.78e-11 at n = 1000) and the truth case (1.9e-12) of tests/test_gpu_loo_mm_split.py, which prints them. The bound of either comparison is ten times the measured value and
never above BOUND."""
import ctypes as C
import sys

import numpy as np

from tests import host_build
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R

TAIL = ("elpd_loo_matched", "khat_split")
BOUND = 1e-9
MEASURED = 1.8e-11
GPU_MEASURED = 4.8e-11


def fields(Cc):
    return R.fields(Cc) + 2


def exact_fields(Cc):
    return X.fields(Cc) + 1


# ---- the statistic

def split_weights(gene, s, A, B, r_eff):
    """steps 2 - 6: (log weights [n], khat_split, the cell's log-likelihood at the proposal points [n], the proposal points
    [C + 1, n]) for the state (A, B)"""
    T = np.asarray(gene["T"], np.float64)
    nc, n = T.shape
    h = n // 2
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    use = np.array([R.is_coord(gene, c) for c in range(nc)])
    Ainv = np.where(use, 1.0 / A, 1.0)
    Binv = np.where(use, -B / A, 0.0)
    log_j = float(np.sum(np.log(A[use])))
    q_t, ll_t = R.local_density(gene, A, B)
    q_0, ll_0 = R.local_density(gene, np.ones(nc), np.zeros(nc))
    q_i, _ = R.local_density(gene, Ainv, Binv)
    first = np.arange(n) < h
    qx, llx = np.where(first, q_t, q_0), np.where(first, ll_t[s], ll_0[s])
    d = np.where(first, q_0, q_i) - log_j
    with np.errstate(invalid="ignore"):
        r = qx - llx - np.logaddexp(qx, d)
    lw, k = R.psis(np.where(np.isfinite(r), r, -np.inf), r_eff)
    x = np.where(first[None, :], R.transformed(gene, A, B), T)
    return lw, k, llx, x


def point(gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, mm=None):
    """the elpd form: loo_mm_restate.point's dict (mm: a given one in its place) with elpd_loo, p_loo and looic the split ones
    where the cell was matched, and elpd_loo_matched, khat_split"""
    mm = R.point(gene, s, r_eff, k_threshold, max_iters) if mm is None else mm
    out = dict(mm, elpd_loo_matched=mm["elpd_loo"], khat_split=np.nan)
    if mm["iterations"] == 0:
        return out
    lw, k, llx, _ = split_weights(gene, s, mm["scale"], mm["shift"], r_eff)
    part = lw != -np.inf
    if not part.any():
        out.update(elpd_loo=np.nan, p_loo=np.nan, looic=np.nan)
        return out
    nc = gene["T"].shape[0]
    ll0 = R.local_density(gene, np.ones(nc), np.zeros(nc))[1][s]
    ll0 = ll0[ll0 != np.inf]
    lpd = R.L.logsumexp(ll0) - np.log(ll0.size)
    elpd = R.L.logsumexp(lw[part] + llx[part]) - R.L.logsumexp(lw[part])
    out.update(elpd_loo=elpd, p_loo=lpd - elpd, looic=-2.0 * elpd, khat_split=k)
    return out


def as_row(ref):
    """point()'s dict as the [8 + 2 (C + 1)] record of the header"""
    return np.concatenate([R.as_row(ref), [ref[k] for k in TAIL]]).astype(np.float64)


def _err(g, r):
    g, r = float(g), float(r)
    if not np.isfinite(r):
        return 0.0 if (np.isnan(r) and np.isnan(g)) or g == r else np.inf
    return abs(g - r) / max(1.0, abs(r))


def errors(got, ref):
    """the largest error of elpd_loo, khat, scale, shift and khat_split of the elpd form in units of max(1, |ref|); values that
    are not finite must be equal"""
    row = as_row(ref)
    return max(R.errors(got[:-2], row[:-2]), _err(got[-1], row[-1]))


def exact_point(gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, tc=1.0, p_lo=0.025, p_hi=0.975, mm=None):
    """the predictive form: loo_mm_exact_restate.point's dict, for a matched cell under the split weights at the proposal
    points, and khat_split (mm: a given dict in the place of loo_mm_restate.point's)"""
    mm = R.point(gene, s, r_eff, k_threshold, max_iters) if mm is None else mm
    if mm["iterations"] == 0:
        return dict(X.point(gene, s, r_eff, k_threshold, max_iters, tc, p_lo, p_hi), khat_split=np.nan)
    out = {k: np.nan for k in X.HEAD}
    out.update(y=int(gene["y"][s]), excluded=bool(gene["excl"][s]), khat_before=mm["khat_before"], iterations=mm["iterations"],
               scale=np.asarray(mm["scale"], float), shift=np.asarray(mm["shift"], float), kinds=mm.get("kinds"), khat_split=np.nan)
    Cc = gene["X"].shape[1]
    lw, k, _, x = split_weights(gene, s, mm["scale"], mm["shift"], r_eff)
    if not np.isfinite(lw).any():
        return out
    w = np.exp(lw - R.L.logsumexp(lw))
    eta = gene["expo"][s] + np.asarray(gene["X"], float)[s] @ x[:Cc]
    phi = tc * np.exp(-x[Cc])
    with np.errstate(over="ignore", invalid="ignore"):
        mu = np.exp(eta)
    if not (np.all(np.isfinite(eta)) and np.all(np.isfinite(phi)) and np.all(phi > 0) and np.all(np.isfinite(mu))):
        return out
    out.update(X.predictive(w, mu, phi, out["y"], p_lo, p_hi), khat=mm["khat"], khat_split=k, w=w, mu=mu, phi=phi, p_lo=p_lo, p_hi=p_hi)
    return out


def exact_errors(got, ref):
    """the largest error of the predictive form's real fields (loo_mm_exact_restate.errors) and khat_split"""
    return max(X.errors(got[:-1], ref), _err(got[-1], ref["khat_split"]))


# ---- the CPU build of the header

def host_lib():
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    gene = [dp, dp, C.c_long, C.c_int, C.c_int, C.c_int, ip, dp, dp, C.c_double]
    return host_build.host_lib("loo_mm_split_twin", {
        "loo_mm_split_twin_cell": (gene + [C.c_int, C.c_double, C.c_double, C.c_int, dp], None),
        "loo_mm_split_twin_from_record": (gene + [C.c_int, C.c_double, dp, dp], None),
        "loo_mm_split_twin_exact_cell": (gene + [C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, dp], None),
        "loo_mm_split_twin_exact_from_record": (gene + [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, dp, dp], None)})


def host_cell(h, gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30):
    """the cell's record [8 + 2 (C + 1)] of the CPU build"""
    keep, args = R._gene_args(gene)
    out = np.zeros(fields(gene["X"].shape[1]))
    h.loo_mm_split_twin_cell(*args, int(s), float(r_eff), float(k_threshold), int(max_iters), R._dp(out))
    return out


def host_from_record(h, gene, s, rec, r_eff=1.0):
    keep, args = R._gene_args(gene)
    rec = np.ascontiguousarray(rec, np.float64)
    out = np.zeros(fields(gene["X"].shape[1]))
    h.loo_mm_split_twin_from_record(*args, int(s), float(r_eff), R._dp(rec), R._dp(out))
    return out


def host_exact_cell(h, gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, tc=1.0, p_lo=0.025, p_hi=0.975):
    """the cell's record [13 + 2 (C + 1)] of the CPU build"""
    keep, args = R._gene_args(gene)
    out = np.zeros(exact_fields(gene["X"].shape[1]))
    h.loo_mm_split_twin_exact_cell(*args, int(s), float(r_eff), float(k_threshold), int(max_iters), float(tc), float(p_lo), float(p_hi),
                                   R._dp(out))
    return out


def host_exact_from_record(h, gene, s, rec, r_eff=1.0, tc=1.0, p_lo=0.025, p_hi=0.975):
    keep, args = R._gene_args(gene)
    rec = np.ascontiguousarray(rec, np.float64)
    out = np.zeros(exact_fields(gene["X"].shape[1]))
    h.loo_mm_split_twin_exact_from_record(*args, int(s), float(r_eff), float(tc), float(p_lo), float(p_hi), R._dp(rec), R._dp(out))
    return out


def truth_rows(h, xh, truth, n, seeds=(1, 2, 3), label="truth"):
    """the rows of the truth case of tests/loo_mm_cases.py at n draws, printed: per seed the CPU build's matched (h: this
    module's host_lib; xh: loo_mm_exact_restate's, the unsplit predictive) against split figures; truth: cases.truth_elpd()"""
    from tests import loo_mm_cases as cases
    s = cases.TRUTH_CELL
    rows = []
    for seed in seeds:
        gene = cases.gene_of(cases.truth_set(seed, n), 0)
        got, xgot, unsplit = host_cell(h, gene, s), host_exact_cell(h, gene, s), X.host_cell(xh, gene, s)
        row = dict(n=n, seed=seed, qualifies=R.qualifies(gene, s, R.point(gene, s)), iterations=int(got[5]), khat=got[3],
                   khat_split=got[-1], e_matched=abs(got[-2] - truth), e_split=abs(got[0] - truth), upper_matched=unsplit[5],
                   upper_split=xgot[5], mean_matched=unsplit[0], mean_split=xgot[0])
        print(f"{label} {n} {seed} iterations {row['iterations']} khat {row['khat']:.2f} khat_split {row['khat_split']:.2f} "
              f"|elpd_loo - truth| {row['e_matched']:.3f} -> {row['e_split']:.3f} upper {row['upper_matched']:.0f} -> "
              f"{row['upper_split']:.0f} mean {row['mean_matched']:.1f} -> {row['mean_split']:.1f} qualifies {row['qualifies']}", flush=True)
        rows.append(row)
    return rows


def fine_grid(points=2500, n=4000):
    """the truth case on a grid of points x points (DESIGN 8.10 reports the overshoot of repeated shifts at 2500): prints the
    rows that DESIGN 8.13 records. Minutes and gigabytes: a command, not a test."""
    from tests import loo_mm_cases as cases
    cases.TRUTH_GRID = (np.linspace(2.5, 9.5, points), np.linspace(-5.5, 3.0, points))
    truth = cases.truth_elpd()
    print("truth on the grid of", points, "x", points, ":", truth, flush=True)
    return truth_rows(host_lib(), X.host_lib(), truth, n, label=f"grid {points}")


def sanitize():
    """the twin's stand-alone program under the host sanitizers (python -m tests.host_build --sanitize loo_mm_split_twin); its exit status"""
    return host_build.sanitize(["loo_mm_split_twin"])


if __name__ == "__main__":
    if sys.argv[1:] == ["--fine-grid"]:
        fine_grid()
        sys.exit(0)
    if sys.argv[1:] != ["--sanitize"]:
        sys.exit("usage: python -m tests.loo_mm_split_restate --sanitize | --fine-grid")
    sys.exit(sanitize())
