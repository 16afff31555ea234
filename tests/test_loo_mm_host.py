"""Gene-local moment matching of PSIS-LOO cells without a GPU: the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_loo_mm.h: loo_mm_cell_host, tests/loo_mm_host) against the numpy / scipy restatement
(tests/loo_mm_restate.py) on the designed cells of tests/loo_mm_cases.py, the untouched cells against loo_cell_host bit for bit,
the local density against the whole model's log_prob (oracle), and the truth case whose held-out density is known by
quadrature. The modifier of inference.CHECKS is held in tests/test_pass_checks_loo_mm_host.py.

Tolerances. Integer fields (iterations, the accepted candidate kinds) equal, on cases that qualify: the restatement's decisions
are the same under ten perturbations of every ratio by 1e-9 relative (as tests/nuts_cases.py qualifies its own). khat, elpd_loo,
scale and shift: ten times the largest error measured on the designed cases in units of max(1, |ref|) (R.MEASURED,
printed by test_header_matches_restatement), never above 1e-9. The reasoning: a ratio is a difference of sums of at most S + 4
terms below 1e4, so about 1e-11 before k-hat's conditioning, which the qualification bounds.

The truth case (the posterior of one gene on a 900 x 900 grid, the held-out density of an outlying cell by quadrature):
measured errors of elpd_loo, plain PSIS -> matched, seeds 1, 2, 3: n = 1000: 1.543 -> 0.375, 1.418 -> 0.546, 0.660 -> 0.092;
n = 4000: 1.202 -> 0.032, 1.510 -> 0.131, 0.682 -> 0.232; khat 0.84 .. 1.37 -> 0.41 .. 0.69. The largest ratio is 0.39."""
import numpy as np
import pytest

from tests import loo_mm_cases as cases
from tests import loo_mm_restate as R

DESIGNED = cases.designed()


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


def _kw(c):
    return dict(r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"])


def _gene(c):
    return cases.gene_of(cases.draw_set(c["set"]), c["g"])


def test_header_matches_restatement(host):
    worst = 0.0
    for c in DESIGNED:
        gene = _gene(c)
        ref = R.point(gene, c["s"], **_kw(c))
        assert R.qualifies(gene, c["s"], ref, **_kw(c)), c["name"]
        got, kinds = R.host_cell(host, gene, c["s"], **_kw(c))
        assert kinds == ref["kinds"] and got[5] == ref["iterations"] == len(kinds), (c["name"], kinds, ref["kinds"])
        row = R.as_row(ref)
        assert np.array_equal(np.isnan(got), np.isnan(row)) and np.array_equal(np.isinf(got), np.isinf(row)), c["name"]
        err = R.errors(got, row)
        worst = max(worst, err)
        assert err <= min(10 * R.MEASURED, R.BOUND), (c["name"], err)
        for i in (1, 2, 4):                                           # p_loo, looic, khat_before follow from the same sums
            assert np.isnan(row[i]) and np.isnan(got[i]) or abs(got[i] - row[i]) <= R.BOUND * max(1.0, abs(row[i])), (c["name"], i)
    print("largest error of khat, elpd_loo, scale, shift against the restatement:", worst)
    assert worst <= R.MEASURED                                        # the recorded value is the measured one


def test_designed_cells_are_what_they_claim():
    by = {c["name"]: c for c in DESIGNED}
    assert len(by) == len(DESIGNED)
    ref = {name: R.point(_gene(c), c["s"], **_kw(c)) for name, c in by.items()}
    for name, c in by.items():
        if c["kinds"] is not None:
            assert ref[name]["kinds"] == c["kinds"], name
    thr = lambda name: by[name]["k_threshold"]
    assert ref["smooth cell"]["khat"] <= thr("smooth cell")
    r = ref["one shift fixes the outlier"]
    assert r["khat_before"] > 0.7 > r["khat"] and np.all(r["scale"] == 1.0) and np.all(r["shift"] != 0.0)
    for name in ("shift refused, shift and scale accepted (d = 3)", "shift refused, shift and scale accepted (d = 2)"):
        assert 2 in ref[name]["kinds"] and ref[name]["khat"] < thr(name)
    r = ref["shift refused, shift and scale accepted (d = 3)"]
    assert np.all(r["scale"] != 1.0)                                   # the checked gene: intercept, slope and sigma_raw
    r = ref["shift refused, shift and scale accepted (d = 2)"]
    assert r["scale"][1] == 1.0 and r["shift"][1] == 0.0 and r["scale"][0] != 1.0    # a row the gene does not have
    r = ref["neither candidate accepted"]
    assert r["khat"] == r["khat_before"] > thr("neither candidate accepted") and r["iterations"] == 0
    r = ref["stops at max_iters"]
    assert r["iterations"] == 2 and r["khat"] > 0.7                    # it would have gone on
    r = ref["max_iters = 0"]
    assert r["iterations"] == 0 and r["khat"] > 0.7
    c = by["densities that are not finite at some draws"]
    gene = _gene(c)
    q0, _ = R.local_density(gene, np.ones(3), np.zeros(3))
    assert np.sum(q0 == -np.inf) == 10 and ref[c["name"]]["iterations"] > 0
    assert ref[c["name"]]["kinds"] != ref["shift refused, shift and scale accepted (d = 3)"]["kinds"]    # the planted draws matter
    c = by["r_eff = 0.4"]
    assert ref[c["name"]]["khat_before"] != R.point(_gene(c), c["s"])["khat_before"] and ref[c["name"]]["iterations"] > 0
    r = ref["excluded cell"]
    assert np.isnan(r["khat"]) and r["p_loo"] == 0.0 and np.isfinite(r["elpd_loo"])
    assert all(np.isnan(ref["nan cell"][k]) for k in ("elpd_loo", "p_loo", "looic", "khat", "khat_before"))
    assert ref["outlier in the unchecked gene"]["khat_before"] > 0.7 > ref["outlier in the unchecked gene"]["khat"]


def test_skew_normal_kernel_is_scipys():
    """the restatement's own prior term against scipy.stats.skewnorm, up to its constant"""
    from scipy.stats import skewnorm
    x = np.linspace(2.0, 9.0, 50)
    for skew in (-1.0, 0.0, 2.5):
        a = R.log_skew_normal_kernel(x, 6.5, 1.8, skew)
        b = skewnorm.logpdf(x, skew, loc=6.5, scale=1.8)
        assert np.ptp(a - b) < 1e-12


def test_untouched_cells_are_plain_psis_loo(host):
    """every cell of the designed sets that ends with iterations = 0 holds loo_cell_host's four fields bit for bit"""
    seen = 0
    for name in ("b", "c", "nan"):
        ds = cases.draw_set(name)
        for g in range(2):
            gene = cases.gene_of(ds, g)
            for s in range(4):
                for kw in (dict(), dict(max_iters=0), dict(k_threshold=0.2, max_iters=1)):
                    got, kinds = R.host_cell(host, gene, s, **kw)
                    if got[5] != 0:
                        continue
                    _, ll = R.host_density(host, gene, s, np.ones(3), np.zeros(3))
                    plain = R.host_loo_cell(host, ll, excluded=bool(gene["excl"][s]))
                    assert np.array_equal(got[:4], plain, equal_nan=True), (name, g, s, kw)
                    assert np.array_equal(got[4:], np.concatenate([[plain[3], 0.0], np.ones(3), np.zeros(3)]), equal_nan=True)
                    seen += 1
    assert seen >= 40


def test_local_density_is_the_whole_models(host):
    """q(t') - Q0 of the CPU build against log_prob(theta') - log_prob(theta) of the whole model with only the gene's coordinates
    transformed: the factorisation over the genes, exclusions included. |lp| < 1e4, so its rounding is below 1e-11."""
    from oracle.oracle import Oracle
    orc = Oracle()
    worst = 0.0
    for name in ("b", "c"):
        ds = cases.draw_set(name)
        m = orc.model(ds["counts"], ds["X"], ds["expo"], ds["K"], lambda_mu_mu=ds["lambda_mu_mu"], excl=ds["excl"])
        d = cases.dims(2, 2, 1)
        for g, A, B in ((0, [1.2, 0.8, 1.1], [0.3, -0.2, 0.1]), (0, [1.0, 1.0, 1.0], [-0.5, 0.4, 0.0]), (1, [0.9, 1.0, 1.3], [0.2, 0.0, -0.4])):
            gene = cases.gene_of(ds, g)
            s = 3
            q0, _ = R.host_density(host, gene, s, np.ones(3), np.zeros(3))
            q1, _ = R.host_density(host, gene, s, A, B)
            for i in range(0, 1000, 25):
                u = ds["draws"][i]
                v = u.copy()
                v[d["intercept"] + g] = A[0] * u[d["intercept"] + g] + B[0]
                if g == 0:
                    v[d["alpha1"]] = A[1] * u[d["alpha1"]] + B[1]
                v[d["sigma_raw"] + g] = A[2] * u[d["sigma_raw"] + g] + B[2]
                lp0, _ = orc.log_prob_grad(m, u, want_grad=False)
                lp1, _ = orc.log_prob_grad(m, v, want_grad=False)
                assert abs(lp0) < 1e4 and abs(lp1) < 1e4
                err = abs((q1[i] - q0[i]) - (lp1 - lp0))
                worst = max(worst, err)
                assert err <= 1e-9, (name, g, i, q1[i] - q0[i], lp1 - lp0)
    print("largest difference to the whole model's log_prob:", worst)


TRUTH_SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def truth():
    return cases.truth_elpd()


@pytest.mark.parametrize("n", [1000, 4000])
def test_truth_case(host, truth, n):
    assert abs(truth - (-15.342)) < 1e-3
    for seed in TRUTH_SEEDS:
        gene = cases.gene_of(cases.truth_set(seed, n), 0)
        ref = R.point(gene, cases.TRUTH_CELL)
        plain_ref = R.L.loo_point(R.local_density(gene, np.ones(2), np.zeros(2))[1][cases.TRUTH_CELL])
        # the seed qualifies under the restatement alone
        assert ref["khat"] < 0.7 <= ref["khat_before"] and abs(ref["elpd_loo"] - truth) <= 0.5 * abs(plain_ref[0] - truth), (n, seed)
        got, _ = R.host_cell(host, gene, cases.TRUTH_CELL)
        _, ll = R.host_density(host, gene, cases.TRUTH_CELL, np.ones(2), np.zeros(2))
        plain = R.host_loo_cell(host, ll)
        print(n, seed, "error of elpd_loo: plain PSIS", abs(plain[0] - truth), "matched", abs(got[0] - truth), "khat", got[4], "->", got[3],
              "iterations", got[5])
        assert got[3] < 0.7 <= got[4], (n, seed)
        assert abs(got[0] - truth) <= 0.5 * abs(plain[0] - truth), (n, seed)
