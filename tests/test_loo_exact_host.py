"""The exact leave-one-out predictive tails and interval per cell without a GPU: the CPU build of the kernel's header
(ppcseq_amd/csrc/ppcx_loo_exact.h: loo_exact_cell_host, tests/loo_exact_host) against the scipy / numpy restatement
(tests/loo_exact_restate.py) on the designed columns of tests/loo_exact_cases.py -- NUTS and ADVI weights, excluded or not,
r_eff, ties, degenerate tails, non-finite log-likelihoods, the pass-2 settings, invalid parameters --, an excluded NUTS cell
against ppc_exact_cell_host bit for bit, the identity p_le + p_ge - 1 = sum w_i exp(ll_i). The two rows of
inference.CHECKS are held in tests/test_pass_checks_loo_exact_host.py.

Tolerances (loo_exact_restate.check): khat, mean and sd 1e-12 max(1, |ref|), loo_predict_restate.check's rule for weighted sums;
the tails at the bound of tests/test_nbcdf_host.py (TAILS_BOUND relative in the smaller tail, TAILS_ABS absolute in the larger);
interval ends equal. The one-count allowance of ppc_exact_restate.check is used by no designed case.

Measured on the designed cases, CPU build against restatement: the largest error of a weighted sum (khat, mean, sd) is
WEIGHTED_MEASURED of tests/loo_exact_restate.py, printed by test_header_matches_restatement."""
import numpy as np
import pytest

from tests import loo_exact_cases as cases
from tests import loo_exact_restate as R

DESIGNED = cases.designed()
HOST_CASES = [c for c in DESIGNED if c["p_hi"] < 1.0]          # Q(1) is not a finite count: that case is for the entry points' refusal


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


def _kw(c):
    return dict(log_ratio=c["lr"], excluded=c["excluded"], r_eff=c["r_eff"], tc=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])


def test_header_matches_restatement(host):
    used = cells = 0
    worst = 0.0
    for c in HOST_CASES:
        ref = R.point(c["ll"], c["eta"], c["sg"], c["y"], **_kw(c))
        got, it = R.host_cell(host, c["ll"], c["eta"], c["sg"], c["y"], **_kw(c))
        used += R.check(got, ref, c["name"])
        cells += 1
        assert it <= 2048, c["name"]
        if not np.isnan(ref["mean"]):
            worst = max(worst, *R.weighted_errors(got, ref))
            assert got[4] <= got[5] and got[2] + got[3] >= 1.0 - 1e-12, c["name"]
    print("cells", cells, "interval ends that used the one-count allowance", used, "largest error of a weighted sum", worst)
    assert used == 0
    assert worst <= max(R.WEIGHTED_MEASURED * 4, R.WEIGHTED_BOUND)


def test_designed_columns_are_what_they_claim():
    by = {c["name"]: c for c in DESIGNED}
    names = [c["name"] for c in DESIGNED]
    assert len(set(names)) == len(names)
    point = lambda c, **kw: R.point(c["ll"], c["eta"], c["sg"], c["y"], **{**_kw(c), **kw})
    for name in ("nan ll", "-inf ll", "nan ll excluded", "nan eta", "phi = 0", "nan sigma, excluded", "advi: nan a", "advi: nan ll excluded",
                 "advi: no draw takes part", "advi: +inf ll excluded", "advi: -inf ll"):
        ref = point(by[name])
        assert all(np.isnan(ref[k]) for k in ("mean", "sd", "p_le", "p_ge", "lower", "upper", "outside", "khat")), name
        assert ref["y"] == by[name]["y"] and ref["excluded"] == by[name]["excluded"], name
    for name in ("M < 5", "constant tail", "constant column", "one draw", "advi: constant tail"):
        assert point(by[name])["khat"] == np.inf, name
    for name in ("smooth tail n=1000", "r_eff 0.3", "ties inside the tail", "ties straddling the cutoff", "ties from the cutoff up",
                 "advi: ties inside the tail", "advi: ties straddling the cutoff", "pass 2", "weights follow mu"):
        assert np.isfinite(point(by[name])["khat"]), name
    assert point(by["heavy tail"])["khat"] > 0.5
    for name in ("-inf ll excluded", "pass 2, excluded"):         # already held out: the posterior-predictive cell, khat NaN
        ref = point(by[name])
        assert np.isnan(ref["khat"]) and np.isfinite(ref["mean"]), name
    for name in ("advi: excluded n=2000", "advi: -inf ll excluded", "advi: -inf a takes no part, excluded"):
        assert np.isfinite(point(by[name])["khat"]), name        # an ADVI fit weights an excluded cell too: the overall k-hat
    # r_eff decides the tail: another k-hat at r_eff = 1
    assert point(by["r_eff 0.3"])["khat"] != point(by["r_eff 0.3"], r_eff=1.0)["khat"]
    # the tie rule decides which tied draw gets which weight: reversing the tied draws' parameters moves the mean
    for name in ("ties straddling the cutoff", "advi: ties straddling the cutoff"):
        c = by[name]
        r = -c["ll"] if c["lr"] is None else c["lr"] - c["ll"]
        tied = np.nonzero(cases._tied(r))[0]
        assert tied.size == 10
        eta = c["eta"].copy()
        eta[tied] = eta[tied][::-1]
        a, b = point(c)["mean"], R.point(c["ll"], eta, c["sg"], c["y"], **_kw(c))["mean"]
        assert abs(a - b) > 1e-6 * a, name
    # the held-out interval moves away from the posterior one
    c = by["weights follow mu"]
    loo, post = point(c), R.E.point(c["eta"], c["sg"], c["y"], p_lo=c["p_lo"], p_hi=c["p_hi"])
    assert loo["mean"] > 1.2 * post["mean"] and loo["upper"] > post["upper"] and loo["lower"] > post["lower"]
    assert by["pass 2"]["tc"] == R.TC and by["pass 2"]["p_lo"] == R.P2
    assert [c["name"] for c in DESIGNED if c["refused"]] == ["p_lo = 0", "p_hi = 1"]
    assert point(by["p_lo = 0"])["lower"] == 0


def test_excluded_nuts_cell_is_the_posterior_predictive_cell(host):
    seen = 0
    for c in HOST_CASES:
        if c["lr"] is None and c["excluded"]:
            got, _ = R.host_cell(host, c["ll"], c["eta"], c["sg"], c["y"], **_kw(c))
            ref = R.host_ppc_cell(host, c["eta"], c["sg"], c["y"], excluded=True, tc=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])
            if np.isnan(c["ll"]).any():                             # the ratios' NaN rule comes first
                assert np.isnan(got[0]), c["name"]
                continue
            assert np.array_equal(got[:9], ref, equal_nan=True) and np.isnan(got[9]), c["name"]
            seen += not np.isnan(got[0])
    assert seen >= 2


def test_tails_sum_to_one_plus_the_held_out_density(host):
    """P(X <= y) + P(X >= y) - 1 = P(X = y): with ll the cell's own log-pmf and no truncation compensation, p_le + p_ge - 1 is
    sum_i w_i exp(ll_i), the cell's held-out density exp(elpd_loo), within the two tails' absolute bound"""
    rng = np.random.default_rng(77)
    worst = 0.0
    for n, y, r_eff, lr in ((1000, 40, 1.0, None), (3000, 0, 0.5, None), (2000, 150, 1.0, None), (1000, 40, 1.0, rng.normal(0.0, 1.0, 1000))):
        eta, sg = rng.normal(4.0, 0.5, n), rng.normal(-1.0, 0.3, n)
        ll = R.host_log_pmf(host, eta, sg, y)
        got, _ = R.host_cell(host, ll, eta, sg, y, log_ratio=lr, r_eff=r_eff)
        w, _ = R.cell_weights(ll, lr, False, r_eff)
        d = abs(got[2] + got[3] - 1.0 - float(np.sum(w * np.exp(ll))))
        worst = max(worst, d)
        assert d <= 2 * R.TAILS_ABS + 1e-12, (n, y, d)
    print("largest difference", worst)
