"""The exact posterior-predictive tails and interval per cell without a GPU: the CPU build of the kernel's headers
(ppcseq_amd/csrc/ppcx_ppc_exact.h: ppc_exact_cell_host, tests/ppc_exact_host) against the scipy / numpy restatement
(tests/ppc_exact_restate.py) on designed columns: n in {1, 20, 1 000, 4 000}, constant draws (a pure negative binomial, whose
interval ends are scipy.stats.nbinom.ppf), a wide spread of eta, a spread of phi, the pass-2 truncation compensation and
probabilities; a NaN draw; and the consistency of p_le with the predictive sampler.

Tolerances (ppc_exact_restate.check): mean and sd 1e-12 relative; the tails at the bound of tests/test_nbcdf_host.py; interval
ends equal -- one count apart only where the restatement's own F at that count is within that bound of p, for at most 2 % of the
cells."""
import numpy as np
import pytest

from tests import ppc_exact_restate as R

DESIGNED = R.designed()


@pytest.fixture(scope="module")
def host():
    return R.host_lib()


def test_header_matches_restatement(host):
    used = cells = 0
    for c in DESIGNED:
        kw = dict(excluded=c["excluded"], tc=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])
        ref = R.point(c["eta"], c["sg"], c["y"], **kw)
        got, it = R.host_cell(host, c["eta"], c["sg"], c["y"], **kw)
        used += R.check(got, ref, c["name"])
        cells += 1
        assert it <= 2048, c["name"]
        if not np.isnan(got[0]):
            assert got[4] <= got[5] and got[2] + got[3] >= 1.0 - 1e-12, c["name"]
    print("cells", cells, "interval ends that used the one-count allowance", used)
    assert used <= 0.02 * cells


def test_constant_draws_are_the_negative_binomial(host):
    from scipy.stats import nbinom
    seen = 0
    for c in DESIGNED:
        if not c["name"].startswith("constant draws"):
            continue
        got, _ = R.host_cell(host, c["eta"], c["sg"], c["y"], tc=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"])
        phi, mu = np.exp(-c["sg"][0]) * c["tc"], np.exp(c["eta"][0])
        assert got[4] == nbinom.ppf(c["p_lo"], phi, phi / (phi + mu)), c["name"]
        assert got[5] == nbinom.ppf(c["p_hi"], phi, phi / (phi + mu)), c["name"]
        assert abs(got[1] - np.sqrt(mu + mu * mu / phi)) <= 1e-12 * got[1]
        seen += 1
    assert seen == 8


def test_designed_columns_are_what_they_claim():
    by = {c["name"]: c for c in DESIGNED}
    for name in ("nan eta", "phi = 0", "nan sigma"):
        c = by[name]
        ref = R.point(c["eta"], c["sg"], c["y"], excluded=c["excluded"])
        assert np.isnan(ref["mean"]) and ref["y"] == c["y"] and ref["excluded"] == c["excluded"], name
    assert by["y = 2580228"]["y"] == 2580228 and by["y = 0"]["y"] == 0
    assert R.point(by["excluded"]["eta"], by["excluded"]["sg"], 4000, excluded=True, p_lo=R.P2, p_hi=1 - R.P2)["outside"]
    assert {c["eta"].size for c in DESIGNED} >= {1, 20, 1000, 4000}


def test_excluded_flag_changes_nothing_else(host):
    c = next(c for c in DESIGNED if c["name"] == "excluded")
    a, _ = R.host_cell(host, c["eta"], c["sg"], c["y"], excluded=True, p_lo=c["p_lo"], p_hi=c["p_hi"])
    b, _ = R.host_cell(host, c["eta"], c["sg"], c["y"], excluded=False, p_lo=c["p_lo"], p_hi=c["p_hi"])
    assert a[7] == 1.0 and b[7] == 0.0
    assert np.array_equal(np.delete(a, 7), np.delete(b, 7))


def test_p_le_is_consistent_with_the_sampler(host):
    """One cell with n = 4 000 draws: p_le within 5 binomial standard errors of the fraction of 200 000 counts_rng values <= y
    (50 predictive counts per posterior draw from the host build of nb2_log_rng, each on its own Philox address)."""
    rng = np.random.default_rng(12)
    n, reps, y = 4000, 50, 70
    eta, sg = rng.normal(4.0, 0.5, n), rng.normal(-1.0, 0.4, n)
    got, _ = R.host_cell(host, eta, sg, y)
    phi = np.exp(-sg)
    x = np.concatenate([R.host_rng(host, eta, phi, 12345, cell) for cell in range(reps)])
    assert x.size == 200000
    frac = np.mean(x <= y)
    se = np.sqrt(got[2] * (1 - got[2]) / x.size)
    print("p_le", got[2], "sampled", frac, "standard errors", (frac - got[2]) / se)
    assert 0.05 < got[2] < 0.95
    assert abs(frac - got[2]) <= 5 * se
    assert abs(np.mean(x) - got[0]) <= 5 * got[1] / np.sqrt(x.size)


def test_exact_intervals_refusals():
    import pandas as pd
    from ppcseq_amd.methods import identify_outliers
    df = pd.DataFrame(dict(sample=["a", "b"] * 2, symbol=["g1", "g1", "g2", "g2"], value=np.array([1, 2, 3, 4]),
                           PValue=[0.1] * 4, do_check=[True, True, False, False]))
    with pytest.raises(ValueError, match="exact_intervals"):
        identify_outliers(df, transcript="symbol", abundance="value", approximate_posterior_inference=False,
                          exact_intervals=True, _pass=object())
