"""An independent restatement of the exact leave-one-out predictive under the weights of the matching with the covariance step
(ppcseq_amd/csrc/ppcx_loo_mm_cov_exact.h) with numpy and scipy. The matching is tests/loo_mm_cov_restate.point; the split weights
come from np.linalg.inv / slogdet of the FINAL transform (loo_mm_cov_restate.split_weights) -- deliberately not the inverse
accumulated along the accepted steps, which is the header's definition; the mixture and its quantiles are
tests/loo_mm_exact_restate.predictive. Nothing here is shared with the header. It also holds the loader of the CPU build of the
header (tests/loo_mm_cov_exact_cpu) and the runner of that build's stand-alone program under the host sanitizers:

    python -m tests.loo_mm_cov_exact_restate --sanitize

Shared by tests/test_loo_mm_cov_exact_host.py (CPU) and tests/test_gpu_loo_mm_cov_exact.py (device). A gene is the dict of
tests/loo_mm_restate.py.

MEASURED: the largest error of the CPU build against this restatement over tests/loo_mm_cov_exact_cases.CELLS, split both ways,
in mean, sd, p_le, p_ge, khat, khat_before, khat_split, transform and shift, in units of max(1, |ref|), and of p_le / p_ge
relatively where they are below 1e-3 (test_cpu_build_matches_restatement prints it: 6.50e-11). GPU_MEASURED: that of the device
against the CPU build over the cells (3.99e-11), the draw counts (2.9e-11 at n = 1000) and the widths (1.4e-11) of
tests/test_gpu_loo_mm_cov_exact.py, which prints them. The bound of either comparison is ten times the measured value and never
above BOUND."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

from tests import host_build
from tests import loo_mm_cov_restate as V
from tests import loo_mm_exact_restate as E
from tests import loo_mm_restate as R

HEAD = E.HEAD + ("cov_iterations", "khat_split")
REALS = E.REALS + ("khat_split",)
BOUND = 1e-9
MEASURED = 6.6e-11                                    # 6.50e-11 (a cell at C + 1 = 9); DESIGN 8.17 tabulates it per width
GPU_MEASURED = 4.0e-11                                # 3.99e-11 on the cells (C + 1 = 5), 2.9e-11 on the draw counts (n = 1000), 1.4e-11 on the widths


def fields(Cc):
    return len(HEAD) + (Cc + 1) * (Cc + 1) + (Cc + 1)


# ---- the statistic

def point(gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, split=False, tc=1.0, p_lo=0.025, p_hi=0.975, cov=True):
    """dict of the cell's fields, `transform` [C + 1, C + 1], `shift` [C + 1], `kinds` (loo_mm_cov_restate.point's) and, for a cell
    that is a number, what the interval's allowance needs: w, mu, phi, p_lo, p_hi. cov=False: the third candidate switched off."""
    Cc = gene["X"].shape[1]
    nc, n = gene["T"].shape
    mm = V.point(gene, s, r_eff, k_threshold, max_iters, cov=cov)
    y, excluded = int(gene["y"][s]), bool(gene["excl"][s])
    out = {k: np.nan for k in HEAD}
    M, b = np.asarray(mm["transform"], float), np.asarray(mm["shift"], float)
    out.update(y=y, excluded=excluded, khat_before=mm["khat_before"], iterations=mm["iterations"], cov_iterations=mm["cov_iterations"],
               transform=M, shift=b, kinds=mm["kinds"])
    if mm["iterations"] == 0:
        plain = E.point(gene, s, r_eff, k_threshold, 0, tc, p_lo, p_hi)       # max_iters = 0: the plain predictive
        out.update({k: plain[k] for k in E.HEAD[:10]})
        out.update({k: plain[k] for k in ("w", "mu", "phi", "p_lo", "p_hi") if k in plain})
        return out
    t = V.transformed(gene, M, b)
    if split:
        lw, ks, _ = V.split_weights(gene, s, M, b, r_eff)
        khat = mm["khat"]
        t = np.where(np.arange(n) < n // 2, t, np.asarray(gene["T"], float))
    else:
        q, ll_all = V.local_density(gene, M, b)
        Q0, _ = V.local_density(gene, np.eye(nc), np.zeros(nc))
        with np.errstate(invalid="ignore"):
            r = q - Q0 - ll_all[s]
        lw, khat = R.psis(np.where(np.isfinite(r), r, -np.inf), r_eff)
        ks = np.nan
    if not np.isfinite(lw).any():
        return out
    w = np.exp(lw - R.L.logsumexp(lw))
    eta = gene["expo"][s] + np.asarray(gene["X"], float)[s] @ t[:Cc]
    with np.errstate(over="ignore", invalid="ignore"):
        phi = tc * np.exp(-t[Cc])
        mu = np.exp(eta)
    if not (np.all(np.isfinite(eta)) and np.all(np.isfinite(phi)) and np.all(phi > 0) and np.all(np.isfinite(mu))):
        return out
    out.update(E.predictive(w, mu, phi, y, p_lo, p_hi), khat=khat, khat_split=ks, w=w, mu=mu, phi=phi, p_lo=p_lo, p_hi=p_hi)
    return out


def row_dict(row, Cc):
    nc = Cc + 1
    out = dict(zip(HEAD, row[:len(HEAD)]))
    out["transform"] = np.asarray(row[len(HEAD):len(HEAD) + nc * nc]).reshape(nc, nc)
    out["shift"] = np.asarray(row[len(HEAD) + nc * nc:])
    return out


def _err(g, r, tail=False):
    g, r = float(g), float(r)
    if not np.isfinite(r):
        return 0.0 if (np.isnan(r) and np.isnan(g)) or g == r else np.inf
    e = abs(g - r) / max(1.0, abs(r))
    return max(e, abs(g - r) / r) if tail and 0.0 < r < 1e-3 else e


def errors(got, ref):
    """the largest error of mean, sd, p_le, p_ge, khat, khat_before, khat_split, transform and shift of a record `got` against
    point()'s dict (or row_dict of another record) in units of max(1, |ref|), p_le and p_ge also relatively where the reference is
    below 1e-3; values that are not finite must be equal (error 0 or Inf)"""
    worst = max(_err(got[HEAD.index(k)], ref[k], k in ("p_le", "p_ge")) for k in REALS)
    state = np.concatenate([np.asarray(ref["transform"], float).ravel(), np.asarray(ref["shift"], float)])
    return max([worst] + [_err(g, r) for g, r in zip(got[len(HEAD):], state)])


def check_integers(got, ref, bound, what=""):
    """loo_mm_exact_restate.check_integers (the first twelve fields are its record's) and cov_iterations; returns how many ends
    of the interval used the allowance"""
    used = E.check_integers(got, ref, bound, what)
    assert got[HEAD.index("cov_iterations")] == ref["cov_iterations"], (what, got[:len(HEAD)])
    return used


# ---- the CPU build of the header: tests/loo_mm_cov_exact_cpu (a directory whose name host_build.NAMES does not list)

SOURCE = os.path.join(host_build.ROOT, "tests", "loo_mm_cov_exact_cpu", "loo_mm_cov_exact_cpu.cpp")


def host_lib():
    lib = os.path.join(os.path.dirname(SOURCE), "libloo_mm_cov_exact_cpu.so")
    host_build.build(SOURCE, lib)
    h = C.CDLL(lib)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    gene = [dp, dp, C.c_long, C.c_int, C.c_int, C.c_int, ip, dp, dp, C.c_double]
    h.loo_mm_cov_exact_cpu_cell.argtypes = gene + [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp]
    h.loo_mm_cov_exact_cpu_cell.restype = None
    return h


def host_cell(h, gene, s, r_eff=1.0, k_threshold=0.7, max_iters=30, split=False, tc=1.0, p_lo=0.025, p_hi=0.975):
    """the cell's record [14 + (C + 1)^2 + (C + 1)] of the CPU build"""
    keep, args = R._gene_args(gene)
    out = np.zeros(fields(gene["X"].shape[1]))
    h.loo_mm_cov_exact_cpu_cell(*args, int(s), float(r_eff), float(k_threshold), int(max_iters), int(bool(split)), float(tc), float(p_lo),
                                float(p_hi), R._dp(out))
    return out


def sanitize():
    """the stand-alone program of the CPU build under the host sanitizers, as a child process under a time limit; its exit
    status. Nothing is loaded into Python."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "loo_mm_cov_exact_cpu")
        subprocess.check_call(["g++"] + host_build.SANITIZE + ["-o", exe, SOURCE])
        try:
            status = subprocess.run([exe], timeout=host_build.RUN_SECONDS).returncode
        except subprocess.TimeoutExpired:
            status = 124
    print("loo_mm_cov_exact_cpu under -fsanitize=address,undefined: " + ("clean" if status == 0 else f"exit status {status}"))
    return status


if __name__ == "__main__":
    if sys.argv[1:] != ["--sanitize"]:
        sys.exit("usage: python -m tests.loo_mm_cov_exact_restate --sanitize")
    sys.exit(sanitize())
