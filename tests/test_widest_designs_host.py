"""The per-cell statistics at the widest designs the library takes, without a GPU: C = 8 with a continuous covariate and C = 16
(kMaxC: ones and fifteen indicators), the draw sets "columns8" and "columns16" of tests/wide_design_cases.py, and "columns15", the
latter cut down to 15 columns ((C + 1)^2 = 256, the workgroup's size). The CPU builds of ppcx_loo_mm.h, ppcx_loo_mm_exact.h,
ppcx_loo_mm_split.h and ppcx_loo_mm_cov.h against their numpy / scipy restatements on the designed cells of
wide_design_cases.designed(widest=True) and loo_mm_cov_cases.designed(widest=True); the algebra of the accumulated inverse at
d = 9, 16 and 17; the refusal n <= d at d = 9 and 17 and a duplicated coordinate among 17; the cells without a covariance step
against the plain matching's record; the fit-level restatements on the wide sets; and the conditions the device tests of
tests/test_gpu_widest_designs.py rely on (the draw-count cells qualify at every count).

Tolerances. Integer fields and accepted kinds equal on cells that qualify (every designed cell does: the lists' required counts are
asserted); NaN and Inf in the same places; the reals at ten times the largest error measured on these cells in units of
max(1, |ref|) (W.WIDEST_MEASURED, one value per statistic and width; each test prints its own), never above 1e-9. The algebra:
1e-12, as tests/test_loo_mm_cov_host.py; the condition numbers of the final transforms are printed beside it."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_cov_cases as cov_cases
from tests import loo_mm_cov_restate as V
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as S
from tests import ppc_exact_restate as E
from tests import wide_design_cases as W

DESIGNED = W.designed(widest=True)
COV = cov_cases.designed(widest=True)
TC, P_LO, P_HI = 0.7352941, 0.025, 0.975


def _bound(name, what):
    return min(10 * W.WIDEST_MEASURED[name][what], W.BOUND)


@pytest.fixture(scope="module")
def mm_host():
    return R.host_lib()


@pytest.fixture(scope="module")
def exact_host():
    return X.host_lib()


@pytest.fixture(scope="module")
def split_host():
    return S.host_lib()


@pytest.fixture(scope="module")
def cov_host():
    return V.host_lib()


def _kw(c):
    return dict(r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"])


def _gene(c):
    return cases.gene_of(W.draw_set(c["set"]), c["g"])


_REF = {}


def _mm_ref(c):
    """the restatement's point of a plain designed cell, computed once"""
    if c["name"] not in _REF:
        _REF[c["name"]] = R.point(_gene(c), c["s"], **_kw(c))
    return _REF[c["name"]]


def _cov_ref(c, split):
    key = (c["name"], split)
    if key not in _REF:
        _REF[key] = V.point(_gene(c), c["s"], split=split, **_kw(c))
    return _REF[key]


def _same_places(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, got, ref)


def _check_recorded(worst, what):
    """the recorded values are the measured ones, to the two digits kept"""
    for name, w in worst.items():
        rec = W.WIDEST_MEASURED[name][what]
        assert w <= rec and rec - w <= 0.1 * rec, (name, what, w, rec)


def test_draw_sets_are_what_they_claim():
    for name, Cc, S_ in (("columns8", 8, 12), ("columns16", 16, 20), ("columns15", 15, 20)):
        ds = W.draw_set(name)
        assert ds["X"].shape == (S_, Cc) and ds["counts"].shape == (3, S_) and ds["K"] == 2 and ds["draws"].shape[0] == 1000
        d = cases.dims(3, Cc, 2)
        assert ds["draws"].shape[1] == d["D"] == 3 + 3 + 2 + 2 * (Cc - 2) + 3 + 3
        assert np.all(ds["X"][:, 0] == 1.0) and len(ds["excl"]) == 1
        # every column of the unconstrained vector is filled from exactly one place: no column is constant, no two are the same
        assert np.all(ds["draws"].std(axis=0) > 0)
        assert len({ds["draws"][:, j].tobytes() for j in range(d["D"])}) == d["D"]
        g0, g1, g2 = (cases.gene_of(ds, g) for g in range(3))
        assert g0["checked"] and g1["checked"] and not g2["checked"]
        assert np.all(g2["T"][1:Cc] == 0.0)                             # the rows the unchecked gene does not have
        for c in range(1, Cc):                                            # a wrong stride reads another number
            assert abs(g0["T"][c].mean() - g1["T"][c].mean()) > 0.05, (name, c)
            col = ds["draws"][:, cases.slope_index(d, Cc, c, 0)], ds["draws"][:, cases.slope_index(d, Cc, c, 1)]
            assert np.array_equal(col[0], g0["T"][c]) and np.array_equal(col[1], g1["T"][c])
    x8, x16, x15 = (W.draw_set(n)["X"] for n in ("columns8", "columns16", "columns15"))
    cov = x8[:, 7]                                                        # the generic constants path: a centred covariate
    assert abs(cov.sum()) < 1e-12 and (cov > 0).any() and (cov < 0).any() and np.all(cov != np.round(cov))
    assert set(np.unique(x8[:, 1:7])) == {0.0, 1.0}
    for x in (x16, x15):                                                  # what ppcx_model_create takes above 8 columns
        assert set(np.unique(x[:, 1:])) == {0.0, 1.0} and np.all(x[:, 1:].sum(axis=1) <= 1)
        assert np.all(x[:, 1:].sum(axis=0) >= 1) and np.any(x[:, 1:].sum(axis=0) >= 2) and x.shape[0] >= 18
    # the cut: the same design and draws, laid out as a 15-column model has them
    full = W.draw_set("columns16")
    assert np.array_equal(x15, x16[:, :15]) and np.array_equal(W.draw_set("columns15")["counts"], full["counts"])
    for g in range(3):
        a, b = cases.gene_of(W.draw_set("columns15"), g), cases.gene_of(full, g)
        assert np.array_equal(a["T"][:15], b["T"][:15]) and np.array_equal(a["T"][15], b["T"][16]) and np.array_equal(a["U"], b["U"])
    assert (15 + 1) ** 2 == 256 and (16 + 1) ** 2 == 289


def test_plain_designed_cells_are_what_they_claim():
    assert len({c["name"] for c in DESIGNED}) == len(DESIGNED) == 22
    for c in DESIGNED:
        ref = _mm_ref(c)
        assert R.qualifies(_gene(c), c["s"], ref, **_kw(c)), c["name"]   # every cell qualifies: none is left out of a comparison
        assert ref["kinds"] == c["kinds"], (c["name"], ref["kinds"])
    for name in W.WIDEST:
        mine = [(c, _mm_ref(c), _gene(c)) for c in DESIGNED if c["set"] == name]
        checked = [(c, r, g) for c, r, g in mine if c["g"] < W.K]
        assert any(r["kinds"] and set(r["kinds"]) == {1} for c, r, g in checked), name                     # an accepted shift
        assert any(1 in r["kinds"] and 2 in r["kinds"] for c, r, g in checked), name                       # shift and scale
        assert any(c["g"] == 2 and r["iterations"] > 0 for c, r, g in mine), name                          # the unchecked gene
        assert any(np.isnan(r["khat"]) and g["excl"][c["s"]] for c, r, g in mine), name                    # excluded
        assert any(r["khat_before"] <= c["k_threshold"] and r["iterations"] == 0 and not g["excl"][c["s"]] for c, r, g in mine), name
        assert any(r["iterations"] == c["max_iters"] and r["khat"] > c["k_threshold"] for c, r, g in mine), name   # stop at max_iters
        assert any(c["r_eff"] != 1.0 and r["iterations"] > 0 for c, r, g in mine), name
        for c, r, g in mine:
            Cc = g["X"].shape[1]
            if c["g"] == 2:                                               # the rows the gene does not have keep (1, 0)
                assert np.all(r["scale"][1:Cc] == 1.0) and np.all(r["shift"][1:Cc] == 0.0), c["name"]
            elif r["iterations"] > 0:                                     # every one of the d = C + 1 coordinates moved
                assert np.all(r["shift"] != 0.0), c["name"]
                assert np.all(r["scale"] != 1.0) == (2 in r["kinds"]), c["name"]


def _refused_candidate_was_valid(c):
    """at the final state of a path that ended above the threshold before max_iters the covariance candidate exists: it was
    tried and its khat refused, not found invalid"""
    gene, ref = _gene(c), _cov_ref(c, False)
    nc = gene["T"].shape[0]
    q0, _ = V.local_density(gene, np.eye(nc), np.zeros(nc))
    q, ll = V.local_density(gene, ref["transform"], ref["shift"])
    r = q - q0 - ll[c["s"]] if ref["kinds"] else -ll[c["s"]]
    lw, k = R.psis(np.where(np.isfinite(r), r, -np.inf), c["r_eff"])
    assert abs(k - ref["khat"]) <= 1e-12
    return V.cov_candidate(gene, ref["transform"], ref["shift"], np.exp(lw - R.L.logsumexp(lw))) is not None


def test_covariance_designed_cells_are_what_they_claim():
    assert len({c["name"] for c in COV}) == len(COV) == 20
    d17 = d17_later = d9 = d16 = d2 = refused = 0
    for c in COV:
        gene, ref = _gene(c), _cov_ref(c, False)
        assert V.qualifies(gene, c["s"], ref, **_kw(c)), c["name"]       # every cell qualifies: none is left out of a comparison
        assert ref["kinds"] == c["kinds"], (c["name"], ref["kinds"])
        nc, d, k = gene["T"].shape[0], len(V.coords(gene)), ref["kinds"]
        M = ref["transform"]
        if 3 in k:
            later = any(x in (2, 3) for x in k[k.index(3) + 1:])
            d17, d17_later = d17 + (d == 17), d17_later + (d == 17 and later)
            d9, d16 = d9 + (d == 9), d16 + (d == 16)
            if d == 2 and nc == 17:                                       # coordinates at rows 0 and 16, fifteen identity rows between
                d2 += 1
                assert M[16, 0] != 0.0 and M[0, 16] == 0.0 and M[0, 0] != 1.0 and M[16, 16] != 1.0     # L_w L^-1 is lower triangular
                assert np.array_equal(M[1:16], np.eye(17)[1:16]) and np.array_equal(M[:, 1:16], np.eye(17)[:, 1:16])
                assert np.all(ref["shift"][1:16] == 0.0)
            elif d == nc:                                                 # products of L_w L^-1: a full lower triangle, nothing above
                assert np.all(M[np.tril_indices(nc)] != np.eye(nc)[np.tril_indices(nc)]) and np.all(M[np.triu_indices(nc, 1)] == 0.0), c["name"]
        elif ref["khat"] > c["k_threshold"] and len(k) < c["max_iters"] and not gene["excl"][c["s"]]:
            assert gene["T"].shape[1] > d and _refused_candidate_was_valid(c), c["name"]
            refused += 1
    print("kind-3 paths: d = 17", d17, "(with a later 2 or 3:", d17_later, ") d = 9", d9, "d = 16", d16, "d = 2 inside nc = 17", d2,
          "; tried and refused", refused)
    assert d17 >= 2 and d17_later >= 1 and d9 >= 2 and d16 >= 1 and d2 >= 1 and refused >= 1


def test_matching_twin_against_restatement(mm_host):
    worst = dict.fromkeys(W.WIDEST, 0.0)
    for c in DESIGNED:
        gene, ref = _gene(c), _mm_ref(c)
        got, kinds = R.host_cell(mm_host, gene, c["s"], **_kw(c))
        assert kinds == ref["kinds"] and got[5] == ref["iterations"] == len(kinds), (c["name"], kinds, ref["kinds"])
        row = R.as_row(ref)
        assert got.size == R.fields(gene["X"].shape[1]) == row.size
        _same_places(got, row, c["name"])
        err = R.errors(got, row)
        worst[c["set"]] = max(worst[c["set"]], err)
        assert err <= _bound(c["set"], "mm"), (c["name"], err)
        for i in (1, 2, 4):
            assert np.isnan(row[i]) and np.isnan(got[i]) or abs(got[i] - row[i]) <= W.BOUND * max(1.0, abs(row[i])), (c["name"], i)
    print("widest cells: largest error of khat, elpd_loo, scale, shift against the restatement:", worst)
    _check_recorded(worst, "mm")


def test_exact_twin_against_restatement(exact_host):
    worst, allowed = dict.fromkeys(W.WIDEST, 0.0), []
    for c in DESIGNED:
        gene = _gene(c)
        ref = X.point(gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        got = X.host_cell(exact_host, gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        assert got.size == X.fields(gene["X"].shape[1])
        if X.check_integers(got, ref, _bound(c["set"], "exact"), c["name"]):
            allowed.append(c["name"])
        err = X.errors(got, ref)
        worst[c["set"]] = max(worst[c["set"]], err)
        assert err <= _bound(c["set"], "exact"), (c["name"], err)
    print("widest cells: largest error of the predictive under matched weights against the restatement:", worst,
          "; interval ends within the bound of p:", allowed)
    assert len(allowed) <= 1, allowed
    _check_recorded(worst, "exact")


def test_split_twin_against_restatement(split_host):
    worst, allowed, split = dict.fromkeys(W.WIDEST, 0.0), [], 0
    for c in DESIGNED:
        gene, mm = _gene(c), _mm_ref(c)
        Cc = gene["X"].shape[1]
        ref = S.point(gene, c["s"], mm=mm, **_kw(c))
        got = S.host_cell(split_host, gene, c["s"], **_kw(c))
        assert got.size == S.fields(Cc) and got[5] == ref["iterations"], c["name"]
        assert np.isnan(got[-1]) == (ref["iterations"] == 0), c["name"]
        err = S.errors(got, ref)
        xref = S.exact_point(gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, mm=mm, **_kw(c))
        xgot = S.host_exact_cell(split_host, gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        assert xgot.size == S.exact_fields(Cc)
        if X.check_integers(xgot[:-1], xref, _bound(c["set"], "split"), c["name"]):
            allowed.append(c["name"])
        xerr = S.exact_errors(xgot, xref)
        worst[c["set"]] = max(worst[c["set"]], err, xerr)
        assert err <= _bound(c["set"], "split") and xerr <= _bound(c["set"], "split"), (c["name"], err, xerr)
        split += ref["iterations"] > 0
    print("widest cells: split", split, "largest error of the split forms against the restatement:", worst,
          "; interval ends within the bound of p:", allowed)
    assert split >= 16 and len(allowed) <= 1, (split, allowed)
    _check_recorded(worst, "split")


def test_covariance_twin_against_restatement(cov_host):
    worst = dict.fromkeys(("columns8", "columns16", "columns15"), 0.0)
    for c in COV:
        gene = _gene(c)
        for split in (False, True):
            ref = V.as_row(_cov_ref(c, split))
            got, kinds, _ = V.host_cell(cov_host, gene, c["s"], split=split, **_kw(c))
            assert got.size == V.fields(gene["X"].shape[1]) == 9 + gene["T"].shape[0] ** 2 + gene["T"].shape[0]
            assert kinds == c["kinds"] and all(got[i] == ref[i] for i in V.INTS), (c["name"], split, kinds, got[:9], ref[:9])
            _same_places(got, ref, (c["name"], split))
            assert np.isnan(got[8]) == (not split or got[5] == 0), (c["name"], split)
            if not split:
                assert got[7] == got[0] or np.isnan(got[0]), c["name"]
            err = V.errors(got, ref)
            print(c["name"], "split", split, "kinds", kinds, "khat", got[4], "->", got[3], "khat_split", got[8], "error", err)
            worst[c["set"]] = max(worst[c["set"]], err)
            assert err <= _bound(c["set"], "cov"), (c["name"], split, err)
    print("widest cells: largest error of the covariance form against the restatement:", worst)
    _check_recorded(worst, "cov")


def test_algebra_of_the_accumulated_inverse_at_full_width(cov_host):
    """transform @ Minv = I, Minv @ shift + binv = 0 and logJ = slogdet(transform) on every designed cell, to 1e-12 (the
    tolerances of test_one_covariance_step_matches_the_weighted_moments); the condition numbers are printed: the largest
    measured is 11.5 (columns8; 9.1 at d = 17), so 1e-12 needs no statement relative to it; the residuals are at most 6.3e-15"""
    worst, conds, seen = 0.0, {}, set()
    for c in COV:
        gene = _gene(c)
        nc = gene["T"].shape[0]
        got, kinds, inv = V.host_cell(cov_host, gene, c["s"], **_kw(c))
        d = V.row_dict(got, nc - 1)
        e_inv = np.abs(d["transform"] @ inv["Minv"] - np.eye(nc)).max()
        e_binv = np.abs(inv["Minv"] @ d["shift"] + inv["binv"]).max()
        sign, log_j = np.linalg.slogdet(d["transform"])
        cond = np.linalg.cond(d["transform"])
        print(c["name"], "cond", cond, "|transform Minv - I|", e_inv, "|Minv shift + binv|", e_binv, "logJ", inv["logJ"], "slogdet", log_j)
        assert e_inv <= 1e-12 and e_binv <= 1e-12 and sign > 0 and abs(log_j - inv["logJ"]) <= 1e-12, c["name"]
        worst = max(worst, e_inv, e_binv, abs(log_j - inv["logJ"]))
        conds[c["set"]] = max(conds.get(c["set"], 0.0), cond)
        if 3 in kinds:
            seen.add(len(V.coords(gene)))
    print("largest residual of the three identities:", worst, "largest condition number of a final transform per set:", conds)
    assert seen >= {2, 9, 16, 17}
    assert max(conds.values()) < 1e3


def test_one_covariance_step_matches_the_weighted_moments_at_nine_coordinates(cov_host):
    """"d = 9: 3 is the first accepted kind": the matched draws' unweighted mean and covariance are the step's mw and Sigma_w, to
    1e-10 relative to their size (an identity: Tm Sigma Tm^T = Sigma_w), on a 9 x 9 matrix"""
    c = next(c for c in COV if c["kinds"] == [3])
    gene = _gene(c)
    nc = gene["T"].shape[0]
    got, kinds, _ = V.host_cell(cov_host, gene, c["s"], **_kw(c))
    assert kinds == [3] and nc == 9
    d = V.row_dict(got, nc - 1)
    ll = V.local_density(gene, np.eye(nc), np.zeros(nc))[1][c["s"]]
    lw, _ = R.psis(-ll, c["r_eff"])
    w = np.exp(lw - R.L.logsumexp(lw))
    _, mw, _, sig_w = V.moments(gene, np.eye(nc), np.zeros(nc), w)
    t = d["transform"] @ gene["T"] + d["shift"][:, None]
    e_m = np.abs(t.mean(axis=1) - mw).max() / np.abs(mw).max()
    e_c = np.abs(np.cov(t) - sig_w).max() / np.abs(sig_w).max()
    print(c["name"], "mean", e_m, "covariance", e_c)
    assert e_m <= 1e-10 and e_c <= 1e-10, (e_m, e_c)


def _as_diag(got, nc):
    d = V.row_dict(got, nc - 1)
    return np.concatenate([got[:6], np.diag(d["transform"]), d["shift"]])


REFUSAL_THRESHOLD = 0.1


def test_too_few_draws_and_a_duplicated_coordinate_are_refusals(cov_host, mm_host):
    """tests/test_loo_mm_cov_host.test_invalid_candidate_is_a_refusal at d = 17 and d = 9: prefixes of n = d - 1, d, d + 1 draws of
    the outlier cell of gene 0, and the 17-coordinate gene with slope 2 a copy of slope 1 (a singular Sigma and Sigma_w): no
    covariance step, a finite state, and the record is loo_mm_cell_host's. Every one of them ends above the threshold before
    max_iters: candidate 3 was reached.
    Known limit: the record is held to the other twin, and both twins read the one density, prior and eta of ppcx_loo_mm.h, so
    an error there moves both alike and is not seen here; the tests against the restatement are the ones that see it."""
    todo = []
    for name, d in (("columns16", 17), ("columns8", 9)):
        for n in (d - 1, d, d + 1):
            todo.append((f"{name}: n = {n}", cases.gene_of(cases.prefix(W.draw_set(name), n), 0), 5))
    full = W.draw_set("columns16")
    dup = dict(cases.gene_of(full, 0))
    dup["T"] = dup["T"].copy()
    dup["T"][2] = dup["T"][1]
    todo.append(("columns16: duplicated coordinate", dup, 5))
    for what, gene, s in todo:
        nc = gene["T"].shape[0]
        for split in (False, True):
            got, kinds, _ = V.host_cell(cov_host, gene, s, k_threshold=REFUSAL_THRESHOLD, split=split)
            rec, mm_kinds = R.host_cell(mm_host, gene, s, k_threshold=REFUSAL_THRESHOLD)
            print(what, "split", split, "kinds", kinds, "khat", got[4], "->", got[3], "elpd_loo", got[0])
            assert got[6] == 0 and kinds == mm_kinds, (what, kinds, mm_kinds)
            assert got[3] > REFUSAL_THRESHOLD and got[5] < 30, (what, got[3])     # the loop ended at candidate 3, not before it
            flat = _as_diag(got, nc)
            if split and got[5] > 0:
                flat[:3] = [got[7], rec[1], rec[2]]                  # the unsplit estimate; p_loo and looic follow from it
                assert np.isfinite(got[7]) == np.isfinite(rec[0])
            _same_places(flat, rec, what)
            assert max(V._err(a, b) for a, b in zip(flat, rec)) <= W.BOUND, what
            assert np.all(np.isfinite(got[9:])), what                # never a NaN state
            assert np.all(V.row_dict(got, nc - 1)["transform"][~np.eye(nc, dtype=bool)] == 0.0), what
    # with distinct rows and all the draws the same cell takes covariance steps
    _, kinds, _ = V.host_cell(cov_host, cases.gene_of(full, 0), 5, k_threshold=REFUSAL_THRESHOLD)
    assert 3 in kinds


def test_cells_without_a_covariance_step_are_the_diagonal_records(cov_host, mm_host):
    """every plain designed cell on whose path no kind 3 is accepted gives loo_mm_cell_host's record from loo_mm_cov_cell_host.
    Known limit: one twin is held to the other, and both read the one density, prior and eta of ppcx_loo_mm.h: this test sees what
    the affine state adds (the point, the candidates, the record), not an error in what the twins share, which the tests against
    the restatement see."""
    seen = unmatched = 0
    for c in DESIGNED:
        gene = _gene(c)
        nc = gene["T"].shape[0]
        got, kinds, _ = V.host_cell(cov_host, gene, c["s"], **_kw(c))
        rec, mm_kinds = R.host_cell(mm_host, gene, c["s"], **_kw(c))
        if 3 in kinds:
            print(c["name"], "takes a covariance step:", kinds)
            continue
        seen += 1
        assert kinds == mm_kinds and got[5] == rec[5] and got[6] == 0, (c["name"], kinds, mm_kinds)
        d = V.row_dict(got, nc - 1)
        scale, shift = rec[6:6 + nc], rec[6 + nc:]
        assert np.all(d["transform"][~np.eye(nc, dtype=bool)] == 0.0), c["name"]
        flat = np.concatenate([got[:5], np.diag(d["transform"]), d["shift"]])
        ref = np.concatenate([rec[:5], scale, shift])
        _same_places(flat, ref, c["name"])
        if rec[5] == 0:
            assert np.array_equal(flat, ref, equal_nan=True), c["name"]                # bit for bit
            unmatched += 1
        err = max(V._err(g, r) for g, r in zip(flat, ref))
        assert err <= _bound(c["set"], "cov"), (c["name"], err)
    print("widest cells without a covariance step", seen, "of them unmatched", unmatched)
    assert seen >= 20 and unmatched >= 4


@pytest.mark.parametrize("name,n", [(name, n) for name in cov_cases.WIDEST_COUNTS for n in cov_cases.WIDEST_COUNTS[name]["ns"]])
def test_draw_count_cells_qualify(cov_host, name, n):
    """the two cells per width that the device test holds to the CPU build at its draw counts qualify at every count, and the
    CPU build gives the restatement's record there; at n <= d no covariance step"""
    spec = cov_cases.WIDEST_COUNTS[name]
    ds = cases.prefix(W.draw_set(name), n)
    assert [g for g, s in spec["cells"]] == [spec["cells"][0][0], 2] and spec["cells"][0][0] < W.K     # a checked gene's, the unchecked gene's
    for g, s in spec["cells"]:
        gene = cases.gene_of(ds, g)
        ref = V.point(gene, s, k_threshold=spec["threshold"], split=True)
        assert V.qualifies(gene, s, ref, k_threshold=spec["threshold"]), (name, n, g, s)
        got, kinds, _ = V.host_cell(cov_host, gene, s, k_threshold=spec["threshold"], split=True)
        row = V.as_row(ref)
        assert kinds == ref["kinds"] and all(got[i] == row[i] for i in V.INTS), (name, n, g, s, kinds, ref["kinds"])
        _same_places(got, row, (name, n, g, s))
        err = V.errors(got, row)
        print(name, "n", n, "gene", g, "cell", s, "kinds", kinds, "error", err)
        assert err <= _bound(name, "counts") and err <= W.WIDEST_MEASURED[name]["counts"], (name, n, g, s, err)
        if n <= len(V.coords(gene)):
            assert 3 not in kinds
        if (g, s) == spec["cells"][0] and n >= 255:
            assert 3 in kinds, (name, n, kinds)                           # what the device test asserts at its largest counts


def test_restatements_of_the_fit_level_statistics_stay_within_their_cap():
    """what tests/test_gpu_widest_designs.py asks of Fit.ppc_exact and Fit.loo_predict_exact on the widest draw sets, asked of
    the CPU builds first: eta in numpy from the general-C columns, the restatements' own checks, no interval end on the
    allowance beyond 2 % of the cells"""
    eh, xh = E.host_lib(), XR.host_lib()
    for name in W.WIDEST:
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
