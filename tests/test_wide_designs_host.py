"""The per-cell statistics on designs with more than one slope, without a GPU: the CPU builds of ppcx_loo_mm.h, ppcx_loo_mm_exact.h
and ppcx_loo_mm_split.h against their numpy / scipy restatements on the designed cells of tests/wide_design_cases.py (C = 3 with a
continuous covariate, C = 4 with three indicators; d = 4 and 5 coordinates per checked gene), the local density under a state
that differs in every coordinate, the prior of the slopes c >= 2 on its own, and the conditions the device tests of
tests/test_gpu_wide_designs.py rely on.

Tolerances. Integer fields equal on cases that qualify (loo_mm_restate.qualifies). The reals: ten times the largest error
measured on these cells in units of max(1, |ref|) (W.WIDE_MEASURED, one value per statistic; each test prints its own), never
above 1e-9. The constants recorded for the C <= 2 cells are not used here."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as S
from tests import ppc_exact_restate as E
from tests import wide_design_cases as W

DESIGNED = W.designed()
SETS = ("covariate", "factor4")
TC, P_LO, P_HI = 0.7352941, 0.025, 0.975


def _bound(what):
    return min(10 * W.WIDE_MEASURED[what], W.BOUND)


@pytest.fixture(scope="module")
def mm_host():
    return R.host_lib()


@pytest.fixture(scope="module")
def exact_host():
    return X.host_lib()


@pytest.fixture(scope="module")
def split_host():
    return S.host_lib()


def _kw(c):
    return dict(r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"])


def _gene(c):
    return cases.gene_of(W.draw_set(c["set"]), c["g"])


def _old_gene_of(ds, g):
    """loo_mm_cases.gene_of as it was before it filled the slopes c >= 2"""
    G, S_ = ds["counts"].shape
    Cc = ds["X"].shape[1]
    d = cases.dims(G, Cc, ds["K"])
    u = ds["draws"]
    T = np.zeros((Cc + 1, u.shape[0]))
    T[0] = u[:, d["intercept"] + g]
    if g < ds["K"] and Cc >= 2:
        T[1] = u[:, d["alpha1"] + g]
    T[Cc] = u[:, d["sigma_raw"] + g]
    return T


def test_gene_of_is_unchanged_up_to_two_columns():
    for ds, genes in ((cases.draw_set("b"), 2), (cases.truth_set(1, 50), 1)):
        for g in range(genes):
            assert cases.gene_of(ds, g)["T"].tobytes() == _old_gene_of(ds, g).tobytes()


def test_draw_sets_are_what_they_claim():
    for name, Cc, S_ in (("covariate", 3, 6), ("factor4", 4, 8)):
        ds = W.draw_set(name)
        assert ds["X"].shape == (S_, Cc) and ds["counts"].shape == (3, S_) and ds["K"] == 2 and ds["draws"].shape[0] == 1000
        d = cases.dims(3, Cc, 2)
        assert ds["draws"].shape[1] == d["D"] == 3 + 3 + 2 + 2 * (Cc - 2) + 3 + 3
        assert np.all(ds["X"][:, 0] == 1.0) and len(ds["excl"]) == 1
        # every column of the unconstrained vector is filled from exactly one place
        assert np.all(ds["draws"].std(axis=0) > 0)
        g0, g1, g2 = (cases.gene_of(ds, g) for g in range(3))
        assert g0["checked"] and g1["checked"] and not g2["checked"]
        assert np.all(g2["T"][1:Cc] == 0.0)                             # the rows the unchecked gene does not have
        for c in range(1, Cc):                                            # a wrong stride reads another number
            assert abs(g0["T"][c].mean() - g1["T"][c].mean()) > 0.05, (name, c)
            col = ds["draws"][:, cases.slope_index(d, Cc, c, 0)], ds["draws"][:, cases.slope_index(d, Cc, c, 1)]
            assert np.array_equal(col[0], g0["T"][c]) and np.array_equal(col[1], g1["T"][c])
    cov = W.draw_set("covariate")["X"][:, 2]
    assert abs(cov.sum()) < 1e-12 and (cov > 0).any() and (cov < 0).any() and np.all(cov != np.round(cov))
    assert set(np.unique(W.draw_set("covariate")["X"][:, 1])) == {0.0, 1.0}
    assert set(np.unique(W.draw_set("factor4")["X"][:, 1:])) == {0.0, 1.0}
    long = W.draw_set("long")
    assert long["draws"].shape[0] == 4097 and long["X"].shape == (8, 4)


def test_designed_cells_are_what_they_claim():
    assert len({c["name"] for c in DESIGNED}) == len(DESIGNED)
    ref = {c["name"]: R.point(_gene(c), c["s"], **_kw(c)) for c in DESIGNED}
    for c in DESIGNED:
        assert R.qualifies(_gene(c), c["s"], ref[c["name"]], **_kw(c)), c["name"]
        if c["kinds"] is not None:
            assert ref[c["name"]]["kinds"] == c["kinds"], (c["name"], ref[c["name"]]["kinds"])
    for name in SETS:
        mine = [c for c in DESIGNED if c["set"] == name]
        kinds = [k for c in mine for k in ref[c["name"]]["kinds"]]
        assert 1 in kinds and 2 in kinds, name
        assert any(c["g"] == 2 and ref[c["name"]]["iterations"] > 0 for c in mine), name
        assert any(np.isnan(ref[c["name"]]["khat"]) and _gene(c)["excl"][c["s"]] for c in mine), name
        assert any(ref[c["name"]]["khat_before"] <= c["k_threshold"] and ref[c["name"]]["iterations"] == 0 and not _gene(c)["excl"][c["s"]]
                   for c in mine), name
        for c in mine:
            r, Cc = ref[c["name"]], _gene(c)["X"].shape[1]
            if c["g"] == 2:                                               # the rows the gene does not have keep (1, 0)
                assert np.all(r["scale"][1:Cc] == 1.0) and np.all(r["shift"][1:Cc] == 0.0), c["name"]
            elif r["iterations"] > 0:                                     # every one of the d = C + 1 coordinates moved
                assert np.all(r["shift"] != 0.0), c["name"]
                assert np.all(r["scale"] != 1.0) == (2 in r["kinds"]), c["name"]
    r = ref["factor4: khat stays above the threshold"]
    assert r["khat_before"] > r["khat"] > 0.7
    r = ref["factor4: stops at max_iters"]
    assert r["iterations"] == 2 and r["khat"] > 0.7
    r = ref["covariate: r_eff = 0.4"]
    c = next(c for c in DESIGNED if c["name"] == "covariate: r_eff = 0.4")
    assert r["iterations"] > 0 and r["khat_before"] != R.point(_gene(c), c["s"])["khat_before"]


def test_matching_twin_against_restatement(mm_host):
    worst = 0.0
    for c in DESIGNED:
        gene = _gene(c)
        ref = R.point(gene, c["s"], **_kw(c))
        got, kinds = R.host_cell(mm_host, gene, c["s"], **_kw(c))
        assert kinds == ref["kinds"] and got[5] == ref["iterations"] == len(kinds), (c["name"], kinds, ref["kinds"])
        row = R.as_row(ref)
        assert got.size == R.fields(gene["X"].shape[1]) == row.size
        assert np.array_equal(np.isnan(got), np.isnan(row)) and np.array_equal(np.isinf(got), np.isinf(row)), c["name"]
        err = R.errors(got, row)
        worst = max(worst, err)
        assert err <= _bound("mm"), (c["name"], err)
        for i in (1, 2, 4):
            assert np.isnan(row[i]) and np.isnan(got[i]) or abs(got[i] - row[i]) <= W.BOUND * max(1.0, abs(row[i])), (c["name"], i)
    print("wide cells: largest error of khat, elpd_loo, scale, shift against the restatement:", worst)
    assert worst <= W.WIDE_MEASURED["mm"]                             # the recorded value is the measured one


def test_exact_twin_against_restatement(exact_host):
    worst, allowed = 0.0, []
    for c in DESIGNED:
        gene = _gene(c)
        ref = X.point(gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        got = X.host_cell(exact_host, gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        assert got.size == X.fields(gene["X"].shape[1])
        if X.check_integers(got, ref, _bound("exact"), c["name"]):
            allowed.append(c["name"])
        err = X.errors(got, ref)
        worst = max(worst, err)
        assert err <= _bound("exact"), (c["name"], err)
    print("wide cells: largest error of the predictive under matched weights against the restatement:", worst,
          "; interval ends within the bound of p:", allowed)
    assert len(allowed) <= 1, allowed
    assert worst <= W.WIDE_MEASURED["exact"]


def test_split_twin_against_restatement(split_host):
    worst, allowed, split = 0.0, [], 0
    for c in DESIGNED:
        gene = _gene(c)
        Cc = gene["X"].shape[1]
        mm = R.point(gene, c["s"], **_kw(c))
        ref = S.point(gene, c["s"], mm=mm, **_kw(c))
        got = S.host_cell(split_host, gene, c["s"], **_kw(c))
        assert got.size == S.fields(Cc) and got[5] == ref["iterations"], c["name"]
        assert np.isnan(got[-1]) == (ref["iterations"] == 0), c["name"]
        err = S.errors(got, ref)
        xref = S.exact_point(gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, mm=mm, **_kw(c))
        xgot = S.host_exact_cell(split_host, gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        assert xgot.size == S.exact_fields(Cc)
        if X.check_integers(xgot[:-1], xref, _bound("split"), c["name"]):
            allowed.append(c["name"])
        xerr = S.exact_errors(xgot, xref)
        worst = max(worst, err, xerr)
        assert err <= _bound("split") and xerr <= _bound("split"), (c["name"], err, xerr)
        split += ref["iterations"] > 0
    print("wide cells: split", split, "largest error of the split forms against the restatement:", worst,
          "; interval ends within the bound of p:", allowed)
    assert split >= 10 and len(allowed) <= 1, (split, allowed)
    assert worst <= W.WIDE_MEASURED["split"]


def _state(nc):
    """a state whose A and B differ in every coordinate"""
    c = np.arange(nc)
    return 1.0 + 0.07 * (c + 1) * np.where(c % 2 == 0, 1.0, -1.0), 0.05 * (c + 1) * np.where(c % 2 == 0, -1.0, 1.0)


def _density_error(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))))


def test_density_under_a_state_that_differs_in_every_coordinate(mm_host):
    worst = 0.0
    for name in SETS:
        ds = W.draw_set(name)
        nc = ds["X"].shape[1] + 1
        A, B = _state(nc)
        assert len(set(A)) == nc and len(set(B)) == nc
        for g in range(2):
            gene = cases.gene_of(ds, g)
            q, ll = R.local_density(gene, A, B)
            q0 = R.local_density(gene, np.ones(nc), np.zeros(nc))[0]
            for a, b in [(a, b) for a in range(1, nc - 1) for b in range(a + 1, nc - 1)]:     # two slope rows change states
                A2, B2 = A.copy(), B.copy()
                A2[[a, b]], B2[[a, b]] = A[[b, a]], B[[b, a]]
                moved = np.abs(R.local_density(gene, A2, B2)[0] - q) / np.maximum(1.0, np.abs(q - q0))
                # at more than half of the draws (a draw at which the two rows happen to give the same q shows nothing)
                assert np.median(moved) > 1000 * _bound("density"), (name, g, a, b, np.median(moved))
            for s in range(ds["X"].shape[0]):
                hq, hl = R.host_density(mm_host, gene, s, A, B)
                hq0, _ = R.host_density(mm_host, gene, s, np.ones(nc), np.zeros(nc))
                # q is defined up to the terms without the gene's coordinates: what a ratio reads is q - Q0
                worst = max(worst, _density_error(hq - hq0, q - q0), _density_error(hl, ll[s]))
    print("wide genes: largest error of the local density and the cell's log-likelihood under the state:", worst)
    assert worst <= _bound("density")
    assert worst <= W.WIDE_MEASURED["density"]


def test_prior_of_the_further_slopes_on_its_own(mm_host):
    """with X zero in every slope column no cell reads a slope: two states that differ in one coordinate c >= 2 only differ in
    that slope's prior, the normal of sd 2.5, and in nothing else"""
    from scipy.stats import norm
    seen = 0
    for name in SETS:
        ds = dict(W.draw_set(name))
        X0 = ds["X"].copy()
        X0[:, 1:] = 0.0
        ds["X"] = X0
        nc = X0.shape[1] + 1
        for g in range(2):
            gene = cases.gene_of(ds, g)
            for c in range(2, nc - 1):
                A1, B1 = _state(nc)
                A2, B2 = A1.copy(), B1.copy()
                A2[c], B2[c] = 0.6, 1.9
                t1, t2 = A1[c] * gene["T"][c] + B1[c], A2[c] * gene["T"][c] + B2[c]
                want = norm.logpdf(t1, 0.0, 2.5) - norm.logpdf(t2, 0.0, 2.5)
                assert np.median(np.abs(want)) > 1e-2                  # the two states are told apart
                ref = R.local_density(gene, A1, B1)[0] - R.local_density(gene, A2, B2)[0]
                got = R.host_density(mm_host, gene, 0, A1, B1)[0] - R.host_density(mm_host, gene, 0, A2, B2)[0]
                assert np.abs(ref - want).max() <= 1e-11, (name, g, c)    # |q| < 1e3: differences round below 1e-12
                assert np.abs(got - want).max() <= 1e-11, (name, g, c, np.abs(got - want).max())
                seen += 1
    assert seen == 2 * (1 + 2)


def test_restatements_of_the_fit_level_statistics_stay_within_their_cap():
    """what tests/test_gpu_wide_designs.py asks of Fit.ppc_exact and Fit.loo_predict_exact on the wide draw sets, asked of the
    CPU builds first: eta in numpy from the general-C columns, the restatements' own checks, no interval end on the allowance
    beyond 2 % of the cells"""
    eh, xh = E.host_lib(), XR.host_lib()
    for name in SETS:
        ds = W.draw_set(name)
        eta, sg = W.columns(ds, lambda idx: ds["draws"][:, idx])
        G_, S_ = ds["counts"].shape
        excl = np.isin(np.arange(G_ * S_), ds["excl"]).reshape(G_, S_)
        used = xused = cells = 0
        for g in range(ds["K"]):
            gene = cases.gene_of(ds, g)
            for s in range(S_):
                y = int(ds["counts"][g, s])
                assert np.allclose(eta[:, g, s], ds["expo"][s] + ds["X"][s] @ gene["T"][:-1], rtol=0, atol=1e-13)
                kw = dict(tc=E.TC, p_lo=E.P2, p_hi=1 - E.P2)
                got, _ = E.host_cell(eh, eta[:, g, s], sg[:, g], y, **kw)
                used += E.check(got, E.point(eta[:, g, s], sg[:, g], y, **kw), (name, g, s))
                ll = XR.host_log_pmf(xh, eta[:, g, s], sg[:, g], y)
                xgot, _ = XR.host_cell(xh, ll, eta[:, g, s], sg[:, g], y, excluded=bool(excl[g, s]), **kw)
                xused += XR.check(xgot, XR.point(ll, eta[:, g, s], sg[:, g], y, excluded=bool(excl[g, s]), **kw), (name, g, s))
                cells += 1
        print(name, "cells", cells, "interval ends on the allowance: ppc_exact", used, "loo_predict_exact", xused)
        assert used <= 0.02 * cells and xused <= 0.02 * 2 * cells
