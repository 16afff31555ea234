"""The split transformation of gene-local moment matching without a GPU: the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_loo_mm_split.h: loo_mm_split_cell_host, loo_mm_exact_split_cell_host; tests/loo_mm_split_twin) against the
numpy / scipy restatement (tests/loo_mm_split_restate.py) on the designed cells of tests/loo_mm_cases.py; the cells that are not
matched against the CPU builds of loo_mm_cell_host / loo_mm_exact_cell_host bit for bit; the half boundaries; a record whose one
step moved nothing, which must give plain PSIS; and the truth case, whose held-out density and predictive distribution are
known by quadrature. The two modifiers of inference.MODIFIERS are held in tests/test_pass_checks_loo_mm_split_host.py.

Tolerances. Integer fields equal on cases that qualify (loo_mm_restate.qualifies); an interval end may be one count apart where
the restatement's own F at the count between is within the bound of p, on at most one of the twelve cells. The reals: ten times
the largest error measured on the designed cases (S.MEASURED, printed by test_header_matches_restatement), never above 1e-9.

The truth case (cell 5 of loo_mm_cases.truth_set; truth by quadrature: elpd_loo -15.342, mean 147.03, 97.5 % quantile 325), the
CPU build, matched -> split (test_truth_case prints the rows):
  n     seed  |elpd_loo - truth|  upper       mean            khat_split
  1000  1     0.375 -> 0.004      327 -> 326  146.9 -> 147.1  0.75
  1000  2     0.546 -> 0.018      322 -> 326  146.7 -> 146.8  0.64
  1000  3     0.092 -> 0.027      327 -> 325  146.4 -> 147.4  0.48
  4000  1     0.032 -> 0.010      325 -> 325  147.2 -> 148.2  0.77
  4000  2     0.131 -> 0.098      332 -> 330  149.5 -> 149.8  0.67
  4000  3     0.232 -> 0.012      328 -> 325  147.1 -> 146.4  0.44
The same on a 2500 x 2500 grid at n = 4000 is printed by `python -m tests.loo_mm_split_restate --fine-grid` and recorded in
DESIGN 8.13; nothing of it is asserted."""
import numpy as np
import pytest

from tests import loo_mm_cases as cases
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as S

DESIGNED = cases.designed()
TC, P_LO, P_HI = 0.7352941, 0.025, 0.975
BOUND = min(10 * S.MEASURED, S.BOUND)


@pytest.fixture(scope="module")
def host():
    return S.host_lib()


@pytest.fixture(scope="module")
def mm_host():
    return R.host_lib()


@pytest.fixture(scope="module")
def exact_host():
    return X.host_lib()


def _kw(c):
    return dict(r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"])


def _gene(c):
    return cases.gene_of(cases.draw_set(c["set"]), c["g"])


def test_header_matches_restatement(host):
    assert len(DESIGNED) == 12
    worst, allowed, split = 0.0, [], 0
    for c in DESIGNED:
        gene = _gene(c)
        Cc = gene["X"].shape[1]
        mm = R.point(gene, c["s"], **_kw(c))
        assert R.qualifies(gene, c["s"], mm, **_kw(c)), c["name"]
        # ---- the elpd form
        ref = S.point(gene, c["s"], mm=mm, **_kw(c))
        got = S.host_cell(host, gene, c["s"], **_kw(c))
        assert got[5] == ref["iterations"], c["name"]
        err = S.errors(got, ref)
        assert np.isnan(got[-1]) == (ref["iterations"] == 0), c["name"]
        # ---- the predictive form
        xref = S.exact_point(gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        xgot = S.host_exact_cell(host, gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        assert xgot.size == X.fields(Cc) + 1
        if X.check_integers(xgot[:-1], xref, BOUND, c["name"]):
            allowed.append(c["name"])
        xerr = S.exact_errors(xgot, xref)
        print(c["name"], "iterations", got[5], "khat", got[3], "khat_split", got[-1], "error", err, "predictive", xerr)
        worst = max(worst, err, xerr)
        assert err <= BOUND and xerr <= BOUND, (c["name"], err, xerr)
        split += ref["iterations"] > 0
    print("cells split", split, "largest error against the restatement:", worst, "; interval ends within the bound of p:", allowed)
    assert split >= 6 and len(allowed) <= 1, (split, allowed)
    assert worst <= S.MEASURED                                        # the recorded value is the measured one


def test_designed_cells_show_the_log_jacobian():
    """both "shift and scale accepted" cells end with scales away from 1: with logJ left out of the mixture their ratios move by
    a twentieth and more, far beyond the bound"""
    seen = 0
    for c in DESIGNED:
        if "shift and scale accepted" in c["name"]:
            gene = _gene(c)
            mm = R.point(gene, c["s"], **_kw(c))
            use = np.array([R.is_coord(gene, k) for k in range(gene["T"].shape[0])])
            log_j = np.sum(np.log(mm["scale"][use]))
            print(c["name"], "kinds", mm["kinds"], "logJ", log_j)
            assert 2 in mm["kinds"] and abs(log_j) > 0.05, (c["name"], log_j)
            seen += 1
    assert seen == 2


def test_unmatched_cells_are_the_unsplit_records(host, mm_host, exact_host):
    """every cell that ends with iterations = 0 holds loo_mm_cell_host's / loo_mm_exact_cell_host's record bit for bit, with
    elpd_loo_matched = elpd_loo and khat_split NaN; every cell holds the matching's khat, khat_before, iterations, scale and shift"""
    seen = matched = 0
    for name in ("b", "c", "nan"):
        ds = cases.draw_set(name)
        for g in range(2):
            gene = cases.gene_of(ds, g)
            f, xf = R.fields(gene["X"].shape[1]), X.fields(gene["X"].shape[1])
            for s in range(4):
                for kw in (dict(), dict(max_iters=0), dict(k_threshold=0.2, max_iters=1, r_eff=0.6)):
                    got = S.host_cell(host, gene, s, **kw)
                    xgot = S.host_exact_cell(host, gene, s, tc=TC, p_lo=P_LO, p_hi=P_HI, **kw)
                    rec, _ = R.host_cell(mm_host, gene, s, **kw)
                    xrec = X.host_cell(exact_host, gene, s, tc=TC, p_lo=P_LO, p_hi=P_HI, **kw)
                    assert np.array_equal(got[3:f], rec[3:], equal_nan=True), (name, g, s, kw)
                    assert np.array_equal(got[f:f + 1], rec[:1], equal_nan=True), (name, g, s, kw)
                    assert np.array_equal(xgot[10:xf], xrec[10:], equal_nan=True), (name, g, s, kw)
                    assert np.array_equal(xgot[6:8], xrec[6:8], equal_nan=True), (name, g, s, kw)
                    if rec[5] != 0:
                        matched += 1
                        assert np.isnan(xgot[0]) or xgot[9] == rec[3], (name, g, s, kw)     # khat stays the matching's final k
                        continue
                    assert np.array_equal(got[:f], rec, equal_nan=True) and np.isnan(got[f + 1]), (name, g, s, kw)
                    assert np.array_equal(xgot[:xf], xrec, equal_nan=True) and np.isnan(xgot[xf]), (name, g, s, kw)
                    seen += 1
    assert seen >= 40 and matched >= 8, (seen, matched)


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_half_boundaries(host, n):
    """h = 0, 1, 1 and an odd count on prefixes of the long set: the CPU build against the restatement from a given record of one
    step (scale 1.1 / 0.9, shift 0.05 / -0.1 on the gene's coordinates), and at n = 257 from the matching's own record too"""
    ds = cases.prefix(cases.long_set(), n)
    worst, split = 0.0, 0
    for g in range(2):
        gene = cases.gene_of(ds, g)
        nc = gene["T"].shape[0]
        use = np.array([R.is_coord(gene, k) for k in range(nc)])
        for s in range(4):
            if gene["excl"][s]:
                continue
            todo = []
            plain = R.point(gene, s, max_iters=0)
            given = dict(plain, iterations=1, kinds=[2], scale=np.where(use, np.where(np.arange(nc) % 2 == 0, 1.1, 0.9), 1.0),
                         shift=np.where(use, np.where(np.arange(nc) % 2 == 0, 0.05, -0.1), 0.0))
            rec = R.as_row(given)
            todo.append((given, S.host_from_record(host, gene, s, rec), S.host_exact_from_record(host, gene, s, rec, tc=TC)))
            if n > 3:
                mm = R.point(gene, s)
                assert R.qualifies(gene, s, mm), (n, g, s)
                todo.append((mm, S.host_cell(host, gene, s), S.host_exact_cell(host, gene, s, tc=TC)))
            for mm, got, xgot in todo:
                assert got[5] == mm["iterations"] == xgot[11], (n, g, s)
                ref = S.point(gene, s, mm=mm)
                xref = S.exact_point(gene, s, tc=TC, mm=mm)
                err, xerr = S.errors(got, ref), S.exact_errors(xgot, xref)
                X.check_integers(xgot[:-1], xref, 0.0, (n, g, s))
                worst = max(worst, err, xerr)
                assert err <= BOUND and xerr <= BOUND, (n, g, s, err, xerr)
                assert np.isfinite(got[0]) and np.isfinite(xgot[0]) or mm["iterations"] == 0, (n, g, s)
                split += got[5] > 0
    print("n", n, "cells split", split, "largest error against the restatement", worst)
    assert split >= 7


def test_identity_record_is_plain_psis(host, mm_host):
    """a record with iterations = 1, A = 1, B = 0: both mixture components are the posterior itself, the ratios are -ll - ln 2,
    so elpd_loo and khat_split are plain PSIS's elpd_loo and khat within the measured bound"""
    seen = 0
    for name, g, s, r_eff in (("b", 0, 3, 1.0), ("c", 0, 3, 1.0), ("c", 1, 1, 0.6), ("c", 1, 0, 1.0)):
        gene = cases.gene_of(cases.draw_set(name), g)
        Cc = gene["X"].shape[1]
        plain, _ = R.host_cell(mm_host, gene, s, r_eff=r_eff, max_iters=0)
        rec = plain.copy()
        rec[5] = 1.0
        got = S.host_from_record(host, gene, s, rec, r_eff=r_eff)
        e_elpd = abs(got[0] - plain[0]) / max(1.0, abs(plain[0]))
        e_khat = abs(got[-1] - plain[3]) / max(1.0, abs(plain[3]))
        print(name, g, s, "elpd_loo", got[0], "plain", plain[0], "khat_split", got[-1], "plain khat", plain[3], "errors", e_elpd, e_khat)
        assert e_elpd <= BOUND and e_khat <= BOUND, (name, g, s, e_elpd, e_khat)
        assert got[R.fields(Cc)] == plain[0] and got[3] == plain[3] and got[5] == 1.0
        xgot = S.host_exact_from_record(host, gene, s, rec, r_eff=r_eff, tc=TC)
        xplain = S.host_exact_cell(host, gene, s, r_eff=r_eff, max_iters=0, tc=TC)
        assert abs(xgot[-1] - plain[3]) <= BOUND * max(1.0, abs(plain[3])) and xgot[4] == xplain[4] and xgot[5] == xplain[5]
        assert abs(xgot[0] - xplain[0]) <= BOUND * max(1.0, abs(xplain[0]))
        seen += 1
    assert seen == 4


TRUTH_SEEDS = (1, 2, 3)
TRUTH_UPPER = 325


@pytest.fixture(scope="module")
def truth():
    return cases.truth_elpd()


@pytest.mark.parametrize("n", [1000, 4000])
def test_truth_case(host, exact_host, truth, n):
    assert abs(truth - -15.342) < 1e-3
    for row in S.truth_rows(host, exact_host, truth, n, TRUTH_SEEDS):
        assert row["qualifies"] and row["iterations"] > 0, row
        assert row["e_split"] < row["e_matched"], row
        assert abs(row["upper_split"] - TRUTH_UPPER) <= abs(row["upper_matched"] - TRUTH_UPPER), row
