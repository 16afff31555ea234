"""The exact leave-one-out predictive under moment-matched weights without a GPU: the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_loo_mm_exact.h: loo_mm_exact_cell_host, tests/loo_mm_exact_host) against the numpy / scipy restatement
(tests/loo_mm_exact_restate.py) on the designed cells of tests/loo_mm_cases.py; the cells that are not matched against the CPU
build of loo_exact_cell_host bit for bit; the record of the matching against loo_mm_cell_host bit for bit; and the truth case,
whose held-out predictive distribution is known by quadrature. The modifier of inference.MODIFIERS is held in
tests/test_pass_checks_loo_mm_exact_host.py.

Tolerances. Integer fields equal on cases that qualify (the restatement's accepted candidates are the same under ten
perturbations of every ratio by 1e-9 relative); an interval end may be one count apart where the restatement's own F at the
count between is within the bound of p, on at most one of the twelve cells. The reals: ten times the largest error measured on
the designed cases (X.MEASURED, printed by test_header_matches_restatement), never above 1e-9.

The truth case (cell 5 of loo_mm_cases.truth_set; truth by quadrature: mean 147.03, 2.5 % / 97.5 % quantiles 41 / 325,
P(X >= 900) = 2.454e-5), the CPU build, plain loo_exact_cell_host -> matched:
  n     seed  khat          mean             upper       ln(p_ge / truth)
  1000  1     1.05 -> 0.56  171.8 -> 146.9   410 -> 327  +1.55 -> -0.63
  1000  2     1.20 -> 0.61  185.0 -> 146.7   413 -> 322  +1.42 -> -0.78
  1000  3     1.37 -> 0.45  157.9 -> 146.4   362 -> 327  +0.67 -> -0.05
  4000  1     1.09 -> 0.69  173.9 -> 147.2   398 -> 325  +1.21 -> +0.04
  4000  2     0.84 -> 0.69  180.5 -> 149.5   413 -> 332  +1.51 -> +0.12
  4000  3     1.21 -> 0.41  161.7 -> 147.1   369 -> 328  +0.69 -> +0.18
(test_truth_case prints the rows)."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R

DESIGNED = cases.designed()
TC, P_LO, P_HI = 0.7352941, 0.025, 0.975


@pytest.fixture(scope="module")
def host():
    return X.host_lib()


@pytest.fixture(scope="module")
def exact_host():
    return XR.host_lib()


@pytest.fixture(scope="module")
def mm_host():
    return R.host_lib()


def _kw(c):
    return dict(r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"])


def _gene(c):
    return cases.gene_of(cases.draw_set(c["set"]), c["g"])


def test_header_matches_restatement(host):
    assert len(DESIGNED) == 12
    bound = min(10 * X.MEASURED, X.BOUND)
    worst, allowed = 0.0, []
    for c in DESIGNED:
        gene = _gene(c)
        ref = X.point(gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        assert R.qualifies(gene, c["s"], ref, **_kw(c)), c["name"]
        got = X.host_cell(host, gene, c["s"], tc=TC, p_lo=P_LO, p_hi=P_HI, **_kw(c))
        if X.check_integers(got, ref, bound, c["name"]):
            allowed.append(c["name"])
        err = X.errors(got, ref)
        print(c["name"], "iterations", got[11], "error", err)
        worst = max(worst, err)
        assert err <= bound, (c["name"], err)
    print("largest error against the restatement:", worst, "; interval ends within the bound of p:", allowed)
    assert len(allowed) <= 1, allowed
    assert worst <= X.MEASURED                                        # the recorded value is the measured one


def test_designed_cells_cover_both_paths():
    ref = {c["name"]: X.point(_gene(c), c["s"], tc=TC, **_kw(c)) for c in DESIGNED}
    assert sum(r["iterations"] > 0 for r in ref.values()) >= 6 and sum(r["iterations"] == 0 for r in ref.values()) >= 4
    r = ref["one shift fixes the outlier"]
    plain = X.point(_gene(DESIGNED[1]), DESIGNED[1]["s"], tc=TC, max_iters=0)
    assert r["khat"] < 0.7 < r["khat_before"] == plain["khat"] and (r["upper"], r["mean"]) != (plain["upper"], plain["mean"])
    assert np.isnan(ref["excluded cell"]["khat"]) and np.isfinite(ref["excluded cell"]["mean"]) and ref["excluded cell"]["excluded"]
    assert all(np.isnan(ref["nan cell"][k]) for k in ("mean", "sd", "p_le", "p_ge", "lower", "upper", "outside", "khat", "khat_before"))
    assert ref["densities that are not finite at some draws"]["iterations"] > 0
    assert np.isfinite(ref["densities that are not finite at some draws"]["mean"])


def test_unmatched_cells_are_loo_exact_cell_host(host, exact_host):
    """every cell that ends with iterations = 0 holds the ten fields of the CPU build of loo_exact_cell_host bit for bit"""
    seen = 0
    for name in ("b", "c", "nan"):
        ds = cases.draw_set(name)
        for g in range(2):
            gene = cases.gene_of(ds, g)
            for s in range(4):
                for kw in (dict(), dict(max_iters=0), dict(k_threshold=0.2, max_iters=1, r_eff=0.6)):
                    got = X.host_cell(host, gene, s, tc=TC, p_lo=P_LO, p_hi=P_HI, **kw)
                    if got[11] != 0:
                        continue
                    eta, sg, ll = X.host_columns(host, gene, s)
                    plain, _ = XR.host_cell(exact_host, ll, eta, sg, int(gene["y"][s]), excluded=bool(gene["excl"][s]),
                                            r_eff=kw.get("r_eff", 1.0), tc=TC, p_lo=P_LO, p_hi=P_HI)
                    assert np.array_equal(got[:10], plain, equal_nan=True), (name, g, s, kw)
                    seen += 1
    assert seen >= 40


def test_record_is_loo_mm_cell_host(host, mm_host):
    """khat, khat_before, iterations, scale and shift of every cell are those of loo_mm_cell_host bit for bit"""
    matched = 0
    todo = [(_gene(c), c["s"], _kw(c)) for c in DESIGNED]
    todo += [(cases.gene_of(cases.draw_set(name), g), s, dict()) for name in ("b", "c", "nan") for g in range(2) for s in range(4)]
    for gene, s, kw in todo:
        got = X.host_cell(host, gene, s, tc=TC, **kw)
        rec, _ = R.host_cell(mm_host, gene, s, **kw)
        assert np.array_equal(got[10:], rec[4:], equal_nan=True), (s, kw)
        if np.isnan(got[0]) and rec[5] > 0:
            assert np.isnan(got[9])                                   # the predictive failed: khat goes with it
        else:
            assert np.array_equal(got[9:10], rec[3:4], equal_nan=True), (s, kw, got[9], rec[3])
        matched += rec[5] > 0
    assert matched >= 8


TRUTH_SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def truth():
    return X.truth_predictive()


@pytest.mark.parametrize("n", [1000, 4000])
def test_truth_case(host, exact_host, truth, n):
    assert abs(truth["mean"] - 147.03) < 0.01 and (truth["lower"], truth["upper"]) == (41, 325)
    assert abs(truth["p_ge"] / 2.454e-5 - 1.0) < 1e-3
    s, y = cases.TRUTH_CELL, int(cases.TRUTH_COUNTS[0, cases.TRUTH_CELL])
    for seed in TRUTH_SEEDS:
        gene = cases.gene_of(cases.truth_set(seed, n), 0)
        assert R.qualifies(gene, s, R.point(gene, s)), (n, seed)
        got = X.host_cell(host, gene, s)
        eta, sg, ll = X.host_columns(host, gene, s)
        plain, _ = XR.host_cell(exact_host, ll, eta, sg, y)
        lr = lambda v: np.log(v[3] / truth["p_ge"])
        print(f"{n} {seed} iterations {got[11]:.0f} khat {plain[9]:.2f} -> {got[9]:.2f} mean {plain[0]:.1f} -> {got[0]:.1f} "
              f"upper {plain[5]:.0f} -> {got[5]:.0f} ln(p_ge / truth) {lr(plain):+.2f} -> {lr(got):+.2f}")
        assert got[9] < 0.7 <= got[10] == plain[9], (n, seed)
        assert abs(got[0] - truth["mean"]) <= 0.5 * abs(plain[0] - truth["mean"]), (n, seed)
        assert abs(got[5] - truth["upper"]) <= 0.5 * abs(plain[5] - truth["upper"]), (n, seed)
        assert abs(lr(got)) < abs(lr(plain)), (n, seed)
