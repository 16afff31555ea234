"""ADVI without a GPU: the cases of tests/advi_cases.py qualify, the independent restatement (tests/advi_restate.py) agrees with
oracle.advi on them step for step, and the restatement's own parts hold. tests/test_gpu_advi.py holds the device to the same."""
import math

import numpy as np
import pytest

from oracle import independent as ind
from tests import advi_cases as AC
from tests import advi_restate as R


def _oracle_advi(oracle, case):
    d, excl = case.data()
    mo = oracle.model(d["counts"], d["X"], d["exposure"], case.K, excl=excl)
    return oracle.advi(mo, **case.full_cfg())


@pytest.mark.parametrize("name", list(AC.CASES))
def test_case_qualifies(name):
    """Every perturbed run decides as the unperturbed one, the deciding ELBOs are far apart, Y <= 1e-8; and the case still
    reaches what it was chosen for. A failure here means a library change made the case ill-conditioned: replace its seed."""
    case = AC.CASES[name]
    base, Y, why = AC.qualified(name)
    print(f"case {name}: D = {case.D}, Y = {Y:.3g}" + ("" if base is None else
          f", eta = {base['eta']}, iterations = {base['iterations']}, adaptation ELBOs {base['adapt_elbos']}, "
          f"initial {base['elbo_init']:.6g}"))
    assert why == []
    if case.eta is None:
        assert base is None
    else:
        assert (base["eta"], base["iterations"], base["converged"]) == (case.eta, case.iterations, case.converged)
        assert Y <= AC.Y_MAX


@pytest.mark.parametrize("name", AC.FITTED)
def test_restatement_equals_oracle(oracle, name):
    base, Y, _ = AC.qualified(name)
    ro = _oracle_advi(oracle, AC.CASES[name])
    assert (ro["eta"], ro["iterations"], ro["converged"]) == (base["eta"], base["iterations"], base["converged"])
    dist = AC.distance(ro, base)
    print(f"case {name}: oracle to restatement {dist:.3g}, Y = {Y:.3g}")
    assert dist <= 10 * Y


def test_every_step_size_fails_in_both(oracle):
    assert AC.qualified("H")[0] is None
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        _oracle_advi(oracle, AC.CASES["H"])


def test_restatement_on_an_independent_density(oracle):
    """Case F on torch autograd over the transcribed Stan model (oracle/independent.py) in place of the oracle's C density. The
    two gradients differ by at most 1e-12 (1 + |g|) at the positions the run visits where both are finite (measured: 2e-13), so
    the yardstick Y' is taken at that size, and mu and omega must agree within 10 Y'."""
    case = AC.CASES["F"]
    d, excl = case.data()
    dens_o = AC.oracle_density(oracle, case)
    gap = [0.0]

    def dens_t(z):
        with np.errstate(all="ignore"):
            lp, g = ind.log_prob_grad_torch(z, d["counts"], d["X"], d["exposure"], case.K, excl=excl)
        go = dens_o(z)[1]
        if np.all(np.isfinite(g)) and np.all(np.isfinite(go)):
            gap[0] = max(gap[0], float(np.max(np.abs(g - go) / (1 + np.abs(go)))))
        return lp, g

    rt = AC.run(case, dens_t)
    base, Yp, why = AC.measure(case, dens_o, scale=1e-12)
    print(f"torch to oracle gradient: {gap[0]:.3g}; Y' = {Yp:.3g}")
    assert 0 < gap[0] <= 1e-12 and why == []
    assert (rt["eta"], rt["iterations"]) == (base["eta"], base["iterations"])
    assert np.max(np.abs(rt["mu"] - base["mu"])) <= 10 * Yp
    assert np.max(np.abs(rt["omega"] - base["omega"])) <= 10 * Yp


def _full_log_density(u, counts, X, exposure, K, lambda_mu_mu=5.612671):
    """The model's density on the unconstrained scale from scipy's library densities, every constant kept: log_prob_scipy of
    oracle/independent.py with nothing added back, plus the three Jacobians."""
    from scipy import stats
    G, S = counts.shape
    X = np.asarray(X, float).reshape(S, -1)
    C = X.shape[1]
    o = ind.offsets(G, C, K)
    p = ind.unpack(np.asarray(u, float), G, C, K, lambda_mu_mu)
    lp = u[1] + u[o["sigma_slope"]] + u[o["sigma_sigma"]]
    lp += stats.norm.logpdf(p["lambda_mu"], lambda_mu_mu, 2) + stats.norm.logpdf(p["lambda_sigma"], 0, 2)
    lp += stats.norm.logpdf(p["lambda_skew"], 0, 1) + stats.norm.logpdf(p["sigma_intercept"], 0, 2)
    lp += stats.norm.logpdf(p["sigma_slope"], 0, 2) + stats.norm.logpdf(p["sigma_sigma"], 0, 2)
    lp += np.sum(stats.skewnorm.logpdf(p["intercept"], p["lambda_skew"], loc=p["lambda_mu"] + lambda_mu_mu, scale=p["lambda_sigma"]))
    alpha = np.zeros((C, G))
    alpha[0] = p["intercept"]
    if C >= 2:
        lp += np.sum(stats.laplace.logpdf(p["alpha1"], 0, 1))
        alpha[1, :K] = p["alpha1"]
    if C >= 3:
        lp += np.sum(stats.norm.logpdf(p["alpha2"], 0, 2.5))
        alpha[2:, :K] = p["alpha2"]
    lp += np.sum(stats.norm.logpdf(p["sigma_raw"], p["sigma_slope"] * p["intercept"] + p["sigma_intercept"], p["sigma_sigma"]))
    phi = np.exp(-p["sigma_raw"])[:, None]
    mu = np.exp((X @ alpha).T + np.asarray(exposure)[None, :])
    return float(lp + stats.nbinom.logpmf(counts, phi, phi / (phi + mu)).sum())


@pytest.mark.parametrize("G,S,C,K,seed", [(12, 6, 1, 2, 4), (12, 6, 1, 0, 4), (40, 10, 2, 4, 21), (6, 3, 2, 0, 8), (30, 11, 3, 4, 3),
                                          (30, 11, 3, 0, 3), (25, 9, 5, 6, 5), (25, 9, 5, 0, 5)])
def test_lp_const(oracle, G, S, C, K, seed):
    """The oracle's density (constants of the `~` statements dropped) + lp_const = the full density"""
    d = ind.synth(G, S, K=K, seed=seed, C=C)
    u = np.random.default_rng(seed).uniform(-1, 1, oracle.dim(G, C, K))
    u[3:3 + G] += 5
    mo = oracle.model(d["counts"], d["X"], d["exposure"], K)
    lp = oracle.log_prob_grad(mo, u)[0] + R.lp_const(G, C, K)
    full = _full_log_density(u, d["counts"], d["X"], d["exposure"], K)
    assert abs(lp - full) <= 1e-9 * max(1.0, abs(full)), (lp, full)


# ---- the restatement's own parts

def test_philox_known_answers():
    """The generator's published known-answer vectors (Random123 kat_vectors, philox4x32 with 10 rounds)"""
    def words(c, k):
        return [int(x) for x in R.philox4x32_10(*c, *k)]
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    r = R.philox4x32_10(np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), 0, 0, 0, 0)   # arrays: the scalar result per element
    assert [int(x[0]) for x in r] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_normals_and_initial_point():
    """eta_draw has mean 0 and sd 1 within five standard errors over 1e5 values (even and odd coordinates alone, too); a draw is a
    function of (coordinate, draw, seed) only; the initial point is uniform on (-R, R)."""
    n = 100000
    x = R.eta_draw(n, 17, R.seed32(3))
    for v in (x, x[0::2], x[1::2]):
        assert abs(v.mean()) <= 5 / math.sqrt(v.size)
        assert abs(v.std() - 1) <= 5 / math.sqrt(2 * v.size)
    assert abs(np.mean(x[0::2] * x[1::2])) <= 5 / math.sqrt(n / 2)      # the pair's members are uncorrelated
    assert np.array_equal(R.eta_draw(101, 17, R.seed32(3)), x[:101])
    assert not np.array_equal(R.eta_draw(101, 18, R.seed32(3)), x[:101]) and not np.array_equal(R.eta_draw(101, 17, R.seed32(4)), x[:101])
    q = R.init_point(n, 0, R.seed32(3), 2.0)
    assert np.all(np.abs(q) < 2.0) and abs(q.mean()) <= 5 * (2 / math.sqrt(3)) / math.sqrt(n)
    assert abs(q.std() - 2 / math.sqrt(3)) <= 0.01
    assert not np.array_equal(R.init_point(50, 1, R.seed32(3), 2.0), q[:50])
    assert R.seed32(7) == 7 and R.seed32(1 << 32) == 0x9E3779B9


def test_buffer_rule():
    b = R.RelBuffer(iter=10, eval_elbo=5)            # 0.1 * 10 / 5 < 2: two entries
    assert b.size == 2
    assert R.RelBuffer(iter=50000, eval_elbo=100).size == 50 and R.RelBuffer(iter=400, eval_elbo=20).size == 2
    b.push(1.0)                                      # the first change is against an ELBO of 0: always 1
    assert not b.converged(0.05)
    b.push(0.02)
    assert not b.converged(0.05)                     # mean and median 0.51
    b.push(0.06)                                     # 1.0 left the buffer: mean 0.04
    assert b.v == [0.02, 0.06] and b.converged(0.05) and not b.converged(0.03)
    b = R.RelBuffer(iter=150, eval_elbo=5)           # three entries: the median alone can decide
    for x in (0.001, 10.0, 0.002):
        b.push(x)
    assert b.size == 3 and b.converged(0.005) and not b.converged(0.002)
    b = R.RelBuffer(iter=200, eval_elbo=5)           # four entries: the median is the mean of the middle two
    for x in (0.0, 0.08, 10.0, 0.0):
        b.push(x)
    assert b.converged(0.05) and not b.converged(0.04)
    for x in (9.0, 9.0):
        b.push(x)
    assert b.v == [10.0, 0.0, 9.0, 9.0] and not b.converged(0.05)


@pytest.mark.parametrize("init,elbos,eta,asked", [
    (-50.0, [-10.0, -20.0], 100.0, 2),                       # 10 does worse than 100, and 100 beat the start
    (-50.0, [-math.inf, -10.0, -20.0], 10.0, 3),
    (-50.0, [-math.inf, -math.inf, -10.0, -20.0], 1.0, 4),
    (-50.0, [-math.nan, -math.inf, -80.0, -10.0, -20.0], 0.1, 5),   # not finite counts as -inf; -80 is below the start: go on
    (-50.0, [-60.0, -70.0, -80.0, -90.0, -40.0], 0.01, 5),   # nothing before beat the start; the last one does
    (-50.0, [-10.0, -5.0, -4.0, -3.0, -2.0], 0.01, 5),       # always improving: the last one
    (-50.0, [-60.0, -55.0, -10.0, -9.0, -9.5], 0.1, 5),
    (-50.0, [-60.0, -70.0, -80.0, -90.0, -50.0], None, 5),   # the last one must beat the start strictly
    (-50.0, [-math.inf] * 5, None, 5),
])
def test_adapt_eta_table(init, elbos, eta, asked):
    it = iter(elbos)
    seq = []

    def trial(e):
        seq.append(e)
        return next(it)

    if eta is None:
        with pytest.raises(R.StepSizeError, match="all step sizes failed"):
            R.choose_eta(init, trial)
    else:
        got, seen = R.choose_eta(init, trial)
        assert got == eta and len(seen) == asked
    assert seq == list(R.ETA_SEQUENCE[:asked])


def test_adapt_eta_reports_what_it_compared():
    """The pairs the qualification measures: every trial against the best so far, the best against the start only where the trial
    did worse, the last trial against the start"""
    compared = []
    assert R.choose_eta(-50.0, lambda e, it=iter([-10.0, -20.0]): next(it), compared)[0] == 100.0
    assert compared == [(-10.0, -math.inf), (-20.0, -10.0), (-10.0, -50.0)]
    compared = []
    assert R.choose_eta(-50.0, lambda e, it=iter([-60.0, -70.0, -80.0, -90.0, -40.0]): next(it), compared)[0] == 0.01
    assert compared == [(-60.0, -math.inf), (-70.0, -60.0), (-60.0, -50.0), (-80.0, -70.0), (-70.0, -50.0), (-90.0, -80.0), (-80.0, -50.0),
                        (-40.0, -90.0), (-40.0, -50.0)]
    assert AC.elbo_margin(compared) == pytest.approx(10.0 / 90.0) and AC.elbo_margin([(-math.inf, -math.inf), (-3.0, -math.inf)]) == math.inf
