"""An independent restatement of the gene-local moment matching of the PSIS-LOO cells of an ADVI fit and of the exact predictive
under its weights (ppcseq_amd/csrc/ppcx_loo_mm_ap.h) with numpy and scipy: the local density and the PSIS of
tests/loo_mm_restate.py (local_density / psis), plain approximate-posterior PSIS-LOO of tests/loo_ap_restate.py, the mixture and
its quantiles of tests/loo_mm_exact_restate.predictive. A candidate's log ratio is written as the derivation has it,
a + q(t') - Q0 - ll(t'), left to right -- not in the header's rounding order. Nothing here is shared with the header. It also holds
the loader of the CPU build of the header (tests/loo_mm_ap_cpu) and the runner of that build's stand-alone program under the
host sanitizers:

    python -m tests.loo_mm_ap_restate --sanitize

Shared by tests/test_loo_mm_ap_host.py (CPU) and tests/test_gpu_loo_mm_ap.py (device). A gene is the dict of
tests/loo_mm_restate.py; `a` is [n], the draws' log_p - log_g.

MEASURED: the largest error of the CPU build against this restatement over tests/loo_mm_ap_cases.designed() in khat, elpd_loo,
scale and shift (the elpd form) and in mean, sd, p_le, p_ge, khat, khat_before, scale and shift (the predictive form), in units
of max(1, |ref|) (test_cpu_build_matches_restatement prints both: 2.57e-11). GPU_MEASURED: that of the device against the CPU
build over the designed cells (5.1e-12) and the draw counts of tests/test_gpu_loo_mm_ap.py (1.46e-10 at n = 4 096, in the
predictive form of a cell with two accepted shifts; 1.3e-11 at most at the other counts), which prints them. The bound of either
comparison is ten times the measured value and never above BOUND."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

from tests import host_build
from tests import loo_ap_restate as AP
from tests import loo_mm_exact_restate as E
from tests import loo_mm_restate as R

HEAD = R.HEAD
EXACT_HEAD = E.HEAD
BOUND = 1e-9
MEASURED = 2.6e-11                                    # 2.57e-11 in either form (the d = 3 cell with two scale steps)
GPU_MEASURED = 1.5e-10                                # 1.46e-10 (n = 4 096); the designed cells 5.1e-12


# ---- the statistic

def candidate_ratios(gene, a, s, A, B, Q0):
    """(the log ratios [n] of the state (A, B), -Inf where they are not finite; the cell's log-likelihood at the state)"""
    q, ll = R.local_density(gene, A, B)
    with np.errstate(invalid="ignore"):
        r = a + q - Q0 - ll[s]
    return np.where(np.isfinite(r), r, -np.inf), ll[s]


def point(gene, a, s, k_threshold=0.7, max_iters=30, perturb=None):
    """dict of the cell's fields, `scale` and `shift` [C + 1] and `kinds` (the accepted candidates in order). perturb: None, or
    (rng, rel): every ratio is multiplied by 1 + rel u, u uniform in [-1, 1] (the qualification of a designed case)."""
    a = np.asarray(a, np.float64)
    Cc = gene["X"].shape[1]
    nc = Cc + 1
    n = gene["T"].shape[1]
    A, B = np.ones(nc), np.zeros(nc)
    excluded = bool(gene["excl"][s])
    jig = (lambda r: r) if perturb is None else (lambda r: r * (1.0 + perturb[1] * perturb[0].uniform(-1.0, 1.0, r.size)))
    Q0, ll_all = R.local_density(gene, A, B)
    ll = ll_all[s]
    plain = AP.loo_point(ll, a, excluded)
    out = dict(zip(HEAD, plain + (plain[3], 0)), scale=A.copy(), shift=B.copy(), kinds=[])
    if excluded or max_iters <= 0 or not (plain[3] > k_threshold):
        return out
    lpd = plain[0] + plain[1]
    lw, k = R.psis(jig(AP.ratios(ll, a)), 1.0)
    if perturb is not None and not (k > k_threshold):
        out["kinds"] = None                           # the perturbation moved the cell across the threshold
        return out
    while k > k_threshold and len(out["kinds"]) < max_iters:
        w = np.exp(lw - R.L.logsumexp(lw))
        t = R.transformed(gene, A, B)
        m, v = t.mean(axis=1), t.var(axis=1, ddof=1) if n > 1 else np.full(nc, np.nan)
        mw = (w * t).sum(axis=1)
        vw = (w * t * t).sum(axis=1) - mw * mw
        use = np.array([R.is_coord(gene, c) for c in range(nc)])
        with np.errstate(invalid="ignore", divide="ignore"):
            sc = np.where(use, np.sqrt(vw / v), 1.0)
        cands = [(1, A.copy(), np.where(use, B + (mw - m), B))]
        if np.all(np.isfinite(sc) & (sc > 0)):
            cands.append((2, sc * A, np.where(use, sc * (B - m) + mw, B)))
        for kind, A2, B2 in cands:
            r, _ = candidate_ratios(gene, a, s, A2, B2, Q0)
            lw2, k2 = R.psis(jig(r), 1.0)
            if k2 < k:
                A, B, lw, k = A2, B2, lw2, k2
                out["kinds"].append(kind)
                break
        else:
            break
    if out["kinds"]:
        part = lw != -np.inf
        llf = R.cell_log_lik(gene, R.transformed(gene, A, B))[s]
        elpd = R.L.logsumexp(lw[part] + llf[part]) - R.L.logsumexp(lw[part])
        out.update(elpd_loo=elpd, p_loo=lpd - elpd, looic=-2.0 * elpd, khat=k, iterations=len(out["kinds"]), scale=A, shift=B)
    return out


def qualifies(gene, a, s, ref, k_threshold=0.7, max_iters=30, runs=10, rel=1e-9, seed=5):
    """loo_mm_restate.qualifies for this statistic: the accepted candidate kinds are the same under `runs` perturbations of
    every ratio by `rel` relative"""
    rng = np.random.default_rng(seed)
    return all(point(gene, a, s, k_threshold, max_iters, perturb=(rng, rel))["kinds"] == ref["kinds"] for _ in range(runs))


def exact_point(gene, a, s, k_threshold=0.7, max_iters=30, tc=1.0, p_lo=0.025, p_hi=0.975):
    """loo_mm_exact_restate.point's dict for this statistic: the cell's fields, `scale`, `shift`, `kinds` and, for a cell that is
    a number, what the interval's allowance needs: w, mu, phi, p_lo, p_hi"""
    a = np.asarray(a, np.float64)
    Cc = gene["X"].shape[1]
    mm = point(gene, a, s, k_threshold, max_iters)
    y, excluded = int(gene["y"][s]), bool(gene["excl"][s])
    out = {k: np.nan for k in EXACT_HEAD}
    out.update(y=y, excluded=excluded, khat_before=mm["khat_before"], iterations=mm["iterations"], scale=np.asarray(mm["scale"], float),
               shift=np.asarray(mm["shift"], float), kinds=mm["kinds"])
    A, B = out["scale"], out["shift"]
    if mm["iterations"] == 0:
        ll = R.local_density(gene, A, B)[1][s]
        w = AP.weights(ll, a, excluded)
        if w is None:
            return out
        w, _, khat = w
    else:
        Q0, _ = R.local_density(gene, np.ones(Cc + 1), np.zeros(Cc + 1))
        r, _ = candidate_ratios(gene, a, s, A, B, Q0)
        lw, khat = R.psis(r, 1.0)
        if not np.isfinite(lw).any():
            return out
        w = np.exp(lw - R.L.logsumexp(lw))
    t = R.transformed(gene, A, B)
    eta = gene["expo"][s] + np.asarray(gene["X"], float)[s] @ t[:Cc]
    with np.errstate(over="ignore", invalid="ignore"):
        phi = tc * np.exp(-t[Cc])
        mu = np.exp(eta)
    if not (np.all(np.isfinite(eta)) and np.all(np.isfinite(phi)) and np.all(phi > 0) and np.all(np.isfinite(mu))):
        return out
    out.update(E.predictive(w, mu, phi, y, p_lo, p_hi), khat=khat, w=w, mu=mu, phi=phi, p_lo=p_lo, p_hi=p_hi)
    return out


# ---- the CPU build of the header: tests/loo_mm_ap_cpu (a directory whose name host_build.NAMES does not list)

SOURCE = os.path.join(host_build.ROOT, "tests", "loo_mm_ap_cpu", "loo_mm_ap_cpu.cpp")


def host_lib():
    lib = os.path.join(os.path.dirname(SOURCE), "libloo_mm_ap_cpu.so")
    host_build.build(SOURCE, lib)
    h = C.CDLL(lib)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    gene = [dp, dp, C.c_long, C.c_int, C.c_int, C.c_int, ip, dp, dp, C.c_double]
    h.loo_mm_ap_cpu_cell.argtypes = gene + [dp, C.c_int, C.c_double, C.c_int, dp, ip]
    h.loo_mm_ap_cpu_cell.restype = C.c_int
    h.loo_mm_ap_cpu_exact_cell.argtypes = gene + [dp, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, dp]
    h.loo_mm_ap_cpu_exact_cell.restype = None
    return h


def host_cell(h, gene, a, s, k_threshold=0.7, max_iters=30):
    """(the cell's record [6 + 2 (C + 1)], the accepted kinds) of the CPU build"""
    keep, args = R._gene_args(gene)
    a = np.ascontiguousarray(a, np.float64)
    out = np.zeros(R.fields(gene["X"].shape[1]))
    kinds = np.zeros(max(1, int(max_iters)), np.int32)
    nk = h.loo_mm_ap_cpu_cell(*args, R._dp(a), int(s), float(k_threshold), int(max_iters), R._dp(out),
                              kinds.ctypes.data_as(C.POINTER(C.c_int)))
    return out, kinds[:nk].tolist()


def host_exact_cell(h, gene, a, s, k_threshold=0.7, max_iters=30, tc=1.0, p_lo=0.025, p_hi=0.975):
    """the cell's record [12 + 2 (C + 1)] of the CPU build's predictive form"""
    keep, args = R._gene_args(gene)
    a = np.ascontiguousarray(a, np.float64)
    out = np.zeros(E.fields(gene["X"].shape[1]))
    h.loo_mm_ap_cpu_exact_cell(*args, R._dp(a), int(s), float(k_threshold), int(max_iters), float(tc), float(p_lo), float(p_hi), R._dp(out))
    return out


def sanitize():
    """the stand-alone program of the CPU build under the host sanitizers, as a child process under a time limit; its exit
    status. Nothing is loaded into Python."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "loo_mm_ap_cpu")
        subprocess.check_call(["g++"] + host_build.SANITIZE + ["-o", exe, SOURCE])
        try:
            status = subprocess.run([exe], timeout=host_build.RUN_SECONDS).returncode
        except subprocess.TimeoutExpired:
            status = 124
    print("loo_mm_ap_cpu under -fsanitize=address,undefined: " + ("clean" if status == 0 else f"exit status {status}"))
    return status


if __name__ == "__main__":
    if sys.argv[1:] != ["--sanitize"]:
        sys.exit("usage: python -m tests.loo_mm_ap_restate --sanitize")
    sys.exit(sanitize())
