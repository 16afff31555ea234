"""Gene-local moment matching of the PSIS-LOO cells of an ADVI fit, and the exact predictive under its weights, without a GPU: the
CPU build of the kernels' header (ppcseq_amd/csrc/ppcx_loo_mm_ap.h: loo_mm_ap_cell_host, loo_mm_ap_exact_cell_host;
tests/loo_mm_ap_cpu) against the numpy / scipy restatement (tests/loo_mm_ap_restate.py) on the designed cells of
tests/loo_mm_ap_cases.py; the record against the CPU builds of the sibling headers (ppcx_loo_mm.h with a all zero, ppcx_loo_ap.h
and ppcx_loo_exact.h where nothing was matched, the held-out density p_le + p_ge - 1 against the elpd form); the stand-alone
program under the host sanitizers; and the truth case whose held-out density is known by quadrature. The two modifiers of
inference.MODIFIERS are held in tests/test_pass_checks_loo_mm_ap_host.py.

Tolerances. Integer fields (iterations, the accepted candidate kinds) equal, on cases that qualify: the restatement's decisions
are the same under ten perturbations of every ratio by 1e-9 relative (loo_mm_restate.qualifies' rule). The other fields: ten
times the largest error measured on the designed cases in units of max(1, |ref|) (A.MEASURED, printed by
test_cpu_build_matches_restatement), never above 1e-9, the bound of this family; lower / upper may be one count apart only where
the restatement's own F at the count between them is within the bound of p.

With a all zero: a matched cell's record is ppcx_loo_mm.h's at r_eff = 1 BIT FOR BIT in every field (0 - ll = -ll and Q0 - 0 = Q0
are exact, lpd is formed alike); so are khat and khat_before of an unmatched cell, whose elpd_loo, p_loo and looic are
ppcx_loo_ap.h's -- another order of summation than ppcx_loo.h's -- and agree within 1e-12 max(1, |ref|).

The truth case (loo_mm_ap_cases.truth_ap_set: 1 000 draws of the Gaussian with the grid posterior's marginal moments), error of
elpd_loo against the quadrature, plain approximate-posterior PSIS -> matched, seeds 0 .. 5 (the CPU build; the test prints them):
-0.175 -> +0.282, +0.310 -> -0.061, -0.796 -> -1.156, +0.644 -> +0.177, +0.570 -> -0.012, +0.967 -> -0.165; medians of the absolute
errors 0.607 -> 0.171; khat 1.03 .. 1.50 -> 0.24 .. 0.59. Seed 2 gets worse: the overshoot that the split transformation is for."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import host_build
from tests import loo_exact_restate as XR
from tests import loo_mm_ap_cases as cases
from tests import loo_mm_ap_restate as A
from tests import loo_mm_cases as M
from tests import loo_mm_exact_restate as E
from tests import loo_mm_restate as R

DESIGNED = cases.designed()
BOUND = min(10 * A.MEASURED, A.BOUND)


@pytest.fixture(scope="module")
def host():
    return A.host_lib()


@pytest.fixture(scope="module")
def mm_host():
    return R.host_lib()


def ap_host_lib():
    dp = C.POINTER(C.c_double)
    return host_build.host_lib("loo_ap", {"loo_ap_host_cell": ([dp, dp, C.c_long, C.c_int, dp], None)})


def ap_host_cell(h, ll, a, excluded=False):
    """loo_ap_cell_host's four fields (the CPU build of ppcx_loo_ap.h)"""
    ll, a, out = np.ascontiguousarray(ll, np.float64), np.ascontiguousarray(a, np.float64), np.zeros(4)
    h.loo_ap_host_cell(R._dp(ll), R._dp(a), ll.size, int(excluded), R._dp(out))
    return out


def _kw(c):
    return dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])


def _cell(c):
    ds = cases.draw_set(c["set"])
    return M.gene_of(ds, c["g"]), ds["a"]


def _every_cell():
    """the designed cells, then every cell of the designed sets at three settings"""
    todo = [(_cell(c) + (c["s"], _kw(c))) for c in DESIGNED]
    for name in ("b", "c", "c, -inf", "nan"):
        ds = cases.draw_set(name)
        for g in range(2):
            for s in range(4):
                for kw in (dict(), dict(max_iters=0), dict(k_threshold=0.2, max_iters=1)):
                    todo.append((M.gene_of(ds, g), ds["a"], s, kw))
    return todo


def test_cpu_build_matches_restatement(host):
    assert len(DESIGNED) == 14
    worst, worst_x, allowed = 0.0, 0.0, []
    for c in DESIGNED:
        gene, a = _cell(c)
        ref = A.point(gene, a, c["s"], **_kw(c))
        assert A.qualifies(gene, a, c["s"], ref, **_kw(c)), c["name"]
        got, kinds = A.host_cell(host, gene, a, c["s"], **_kw(c))
        assert kinds == ref["kinds"] and got[5] == ref["iterations"] == len(kinds), (c["name"], kinds, ref["kinds"])
        row = R.as_row(ref)
        assert np.array_equal(np.isnan(got), np.isnan(row)) and np.array_equal(np.isinf(got), np.isinf(row)), c["name"]
        err = R.errors(got, row)
        worst = max(worst, err)
        assert err <= BOUND, (c["name"], err)
        for i in (1, 2, 4):                                           # p_loo, looic, khat_before follow from the same sums
            assert np.isnan(row[i]) and np.isnan(got[i]) or abs(got[i] - row[i]) <= A.BOUND * max(1.0, abs(row[i])), (c["name"], i)
        # the predictive form
        xref = A.exact_point(gene, a, c["s"], **_kw(c))
        xgot = A.host_exact_cell(host, gene, a, c["s"], **_kw(c))
        if E.check_integers(xgot, xref, BOUND, c["name"]):
            allowed.append(c["name"])
        real = [E.HEAD.index(k) for k in E.REALS] + list(range(len(E.HEAD), len(xgot)))
        xrow = np.array([xref[k] for k in E.REALS] + list(xref["scale"]) + list(xref["shift"]), float)
        assert np.array_equal(np.isnan(xgot[real]), np.isnan(xrow)) and np.array_equal(np.isinf(xgot[real]), np.isinf(xrow)), c["name"]
        xerr = E.errors(xgot, xref)
        worst_x = max(worst_x, xerr)
        assert xerr <= BOUND, (c["name"], xerr)
        print(c["name"], "kinds", kinds, "error", err, "of the predictive form", xerr)
    print("largest error against the restatement: the elpd form", worst, "the predictive form", worst_x,
          "; interval ends within the bound of p:", allowed)
    assert len(allowed) <= 1, allowed
    assert max(worst, worst_x) <= A.MEASURED                          # the recorded value is the measured one


def test_designed_cells_are_what_they_claim():
    by = {c["name"]: c for c in DESIGNED}
    assert len(by) == len(DESIGNED)
    ref = {name: A.point(*_cell(c), c["s"], **_kw(c)) for name, c in by.items()}
    overall = {name: R.psis(cases.draw_set(name)["a"], 1.0)[1] for name in ("b", "c")}
    for name, c in by.items():
        if c["kinds"] is not None:
            assert ref[name]["kinds"] == c["kinds"], name
    thr = lambda name: by[name]["k_threshold"]
    assert ref["smooth cell"]["khat"] <= thr("smooth cell")
    r = ref["one shift fixes the outlier"]
    assert r["khat_before"] > 0.7 > r["khat"] and np.all(r["scale"] == 1.0) and np.all(r["shift"] != 0.0)
    r = ref["shift refused, shift and scale accepted (d = 3)"]
    assert 2 in r["kinds"] and np.all(r["scale"] != 1.0)             # the checked gene: intercept, slope and sigma_raw
    r = ref["shift refused, shift and scale accepted (d = 2)"]
    assert r["kinds"][0] == 2 and r["scale"][1] == 1.0 and r["shift"][1] == 0.0 and r["scale"][0] != 1.0    # a row the gene does not have
    r = ref["neither candidate accepted"]
    assert r["khat"] == r["khat_before"] > thr("neither candidate accepted") and r["iterations"] == 0
    r = ref["stops at max_iters"]
    assert r["iterations"] == 2 and r["khat"] > thr("stops at max_iters")    # it would have gone on
    r = ref["max_iters = 0"]
    assert r["iterations"] == 0 and r["khat"] > 0.7
    r = ref["excluded cell"]                                          # loo_approx's record; khat is the overall k-hat of a
    assert r["khat"] == r["khat_before"] == overall["c"] and r["p_loo"] == 0.0 and np.isfinite(r["elpd_loo"]) and r["iterations"] == 0
    for name in ("nan cell", "nan in the log ratios"):
        assert all(np.isnan(ref[name][k]) for k in ("elpd_loo", "p_loo", "looic", "khat", "khat_before")), name
    base = A.point(*_cell(by["stops at max_iters"]), 3)
    r = ref["a = -Inf at some draws"]
    assert np.sum(cases.draw_set("c, -inf")["a"] == -np.inf) == 10 and r["iterations"] > 0 and np.isfinite(r["elpd_loo"])
    assert r["elpd_loo"] != base["elpd_loo"] and r["khat"] != base["khat"]          # ten draws fewer take part
    c = by["densities that are not finite at some draws"]
    gene, a = _cell(c)
    q0, _ = R.local_density(gene, np.ones(3), np.zeros(3))
    assert np.sum(q0 == -np.inf) == 10 and np.array_equal(a == -np.inf, q0 == -np.inf) and np.sum(q0 < -300.0) == 20
    assert ref[c["name"]]["iterations"] > 0 and np.isfinite(ref[c["name"]]["elpd_loo"]) and ref[c["name"]]["khat"] != base["khat"]
    assert ref["outlier in the unchecked gene"]["khat_before"] > 0.7 > ref["outlier in the unchecked gene"]["khat"]
    # a threshold below the overall k-hat: the excluded cell stays above it and unmatched, a live cell is matched all the same
    name = "threshold below the overall k-hat"
    assert thr(name) < overall["c"] and ref[name]["iterations"] > 0 and ref[name]["khat"] < ref[name]["khat_before"]
    excl = A.point(*_cell(by["excluded cell"]), 2, k_threshold=thr(name))
    assert excl["khat"] == overall["c"] > thr(name) and excl["iterations"] == 0


def test_zero_log_ratios_are_the_nuts_statistic(host, mm_host):
    """with a all zero the record is the CPU build of ppcx_loo_mm.h's at r_eff = 1 on the same draws: bit for bit for a matched
    cell; khat and khat_before bit for bit, the other three fields within 1e-12 max(1, |ref|), for an unmatched one (an excluded
    cell aside: a NUTS fit holds it out already)"""
    matched = unmatched = 0
    for name in ("b", "c"):
        ds = cases.draw_set(name)
        zero = np.zeros(ds["draws"].shape[0])
        for g in range(2):
            gene = M.gene_of(ds, g)
            for s in range(4):
                if gene["excl"][s]:
                    continue
                for kw in (dict(), dict(k_threshold=0.2), dict(k_threshold=0.2, max_iters=2)):
                    got, kinds = A.host_cell(host, gene, zero, s, **kw)
                    ref, ref_kinds = R.host_cell(mm_host, gene, s, r_eff=1.0, **kw)
                    assert kinds == ref_kinds, (name, g, s, kw)
                    assert np.array_equal(got[3:], ref[3:]), (name, g, s, kw)
                    if got[5] > 0:
                        assert np.array_equal(got, ref), (name, g, s, kw, got, ref)
                        matched += 1
                    else:
                        assert np.all(np.abs(got[:3] - ref[:3]) <= 1e-12 * np.maximum(1.0, np.abs(ref[:3]))), (name, g, s, kw, got, ref)
                        unmatched += 1
    assert matched >= 10 and unmatched >= 10


def test_unmatched_cells_are_the_plain_approximate_posterior_statistics(host, mm_host):
    """every cell that ends with iterations = 0 holds loo_ap_cell_host's four fields and, in the predictive form,
    loo_exact_cell_host's ten with the log ratios, bit for bit"""
    ap_host, exact_host, diag_host = ap_host_lib(), XR.host_lib(), E.host_lib()
    seen = 0
    for gene, a, s, kw in _every_cell():
        got, _ = A.host_cell(host, gene, a, s, **kw)
        xgot = A.host_exact_cell(host, gene, a, s, tc=0.7352941, **kw)
        assert np.array_equal(xgot[10:], got[4:], equal_nan=True)      # the two forms agree on the matching's record
        if got[5] != 0:
            continue
        excluded = bool(gene["excl"][s])
        _, ll = R.host_density(mm_host, gene, s, np.ones(3), np.zeros(3))
        plain = ap_host_cell(ap_host, ll, a, excluded=excluded)
        assert np.array_equal(got[:4], plain, equal_nan=True), (s, kw)
        assert np.array_equal(got[4:], np.concatenate([[plain[3], 0.0], np.ones(3), np.zeros(3)]), equal_nan=True)
        eta, sg, llx = E.host_columns(diag_host, gene, s)
        xplain, _ = XR.host_cell(exact_host, llx, eta, sg, int(gene["y"][s]), excluded=excluded, log_ratio=a, tc=0.7352941)
        assert np.array_equal(xgot[:10], xplain, equal_nan=True), (s, kw)
        seen += 1
    assert seen >= 50


def test_predictive_form_against_the_elpd_form(host):
    """khat, khat_before, iterations, scale and shift of the two forms are the same bits, and p_le + p_ge - 1 at the observed
    count is exp(elpd_loo) of the elpd form (no truncation compensation), within the two tails' absolute bound"""
    matched, worst = 0, 0.0
    for gene, a, s, kw in _every_cell():
        rec, _ = A.host_cell(host, gene, a, s, **kw)
        got = A.host_exact_cell(host, gene, a, s, **kw)
        assert np.array_equal(got[10:], rec[4:], equal_nan=True), (s, kw)
        assert np.array_equal(got[9:10], rec[3:4], equal_nan=True), (s, kw, got[9], rec[3])
        assert np.isnan(got[0]) == np.isnan(rec[0])
        if np.isnan(rec[0]):
            continue
        d = abs(got[2] + got[3] - 1.0 - np.exp(rec[0]))
        worst = max(worst, d)
        assert d <= 2 * XR.TAILS_ABS + 1e-12, (s, kw, d)
        matched += rec[5] > 0
    print("cells matched", int(matched), "largest |p_le + p_ge - 1 - exp(elpd_loo)|", worst)
    assert matched >= 15


def test_stand_alone_program_is_clean_under_the_host_sanitizers():
    """python -m tests.loo_mm_ap_restate --sanitize: the program is built with -DPPCX_HOST_MAIN and run as a child process;
    nothing sanitised is loaded into Python"""
    out = subprocess.run([sys.executable, "-m", "tests.loo_mm_ap_restate", "--sanitize"], cwd=host_build.ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "clean" in out.stdout


def test_truth_case(host, mm_host):
    truth = M.truth_elpd()
    assert abs(truth - (-15.3423)) < 1e-4
    ap_host = ap_host_lib()
    s = M.TRUTH_CELL
    plain_err, matched_err = [], []
    for seed in cases.TRUTH_SEEDS:
        ds = cases.truth_ap_set(seed)
        gene, a = M.gene_of(ds, 0), ds["a"]
        assert A.qualifies(gene, a, s, A.point(gene, a, s)), seed
        got, kinds = A.host_cell(host, gene, a, s)
        _, ll = R.host_density(mm_host, gene, s, np.ones(2), np.zeros(2))
        plain = ap_host_cell(ap_host, ll, a)
        print(f"seed {seed} error of elpd_loo: plain {plain[0] - truth:+.3f} matched {got[0] - truth:+.3f} khat {got[4]:.2f} -> {got[3]:.2f} "
              f"accepted {kinds}")
        assert got[4] == plain[3] and got[3] < got[4], seed            # the final khat is below khat_before on every seed
        plain_err.append(abs(plain[0] - truth))
        matched_err.append(abs(got[0] - truth))
    print("median |error of elpd_loo|: plain", np.median(plain_err), "matched", np.median(matched_err))
    assert np.median(matched_err) <= np.median(plain_err)
