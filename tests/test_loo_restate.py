"""The PSIS-LOO restatement (tests/loo_restate.py) against answers that do not come from loo's source: the analytic
leave-one-out predictive density of a conjugate normal-mean model, the Pareto shape of normal importance ratios, and the
rules for excluded cells and loo's estimates."""
import math

import numpy as np
import pytest

from tests import loo_restate as L


def _normal_mean_problem(n_obs=30, n_draws=4000, tau=10.0, seed=0):
    """y_i ~ N(mu, 1), mu ~ N(0, tau^2): exact posterior draws and the log-likelihood matrix [n_draws, n_obs]"""
    rng = np.random.default_rng(seed)
    y = rng.normal(size=n_obs)
    y[0] = 4.5                                                  # one observation far in the tail
    prec = 1.0 / tau ** 2 + n_obs
    mu = rng.normal(y.sum() / prec, math.sqrt(1.0 / prec), size=n_draws)
    ll = -0.5 * math.log(2 * math.pi) - 0.5 * (y[None, :] - mu[:, None]) ** 2
    return y, tau, ll


def _analytic_loo(y, tau):
    """log p(y_i | y_-i) = log N(y_i; m_-i, 1 + v_-i), with v_-i = 1 / (1/tau^2 + n - 1), m_-i = v_-i sum_{j != i} y_j"""
    n = y.size
    v = 1.0 / (1.0 / tau ** 2 + n - 1)
    m = v * (y.sum() - y)
    s2 = 1.0 + v
    return -0.5 * math.log(2 * math.pi * s2) - 0.5 * (y - m) ** 2 / s2


def test_elpd_matches_the_analytic_leave_one_out_density():
    y, tau, ll = _normal_mean_problem()
    got = L.loo_columns(ll)
    ref = _analytic_loo(y, tau)
    assert np.all(got[:, 3] < 0.5), got[:, 3]
    # Monte-Carlo error of an importance-sampling estimate at 4 000 draws: well below 0.01 for every cell here
    assert np.max(np.abs(got[:, 0] - ref)) < 0.01, np.abs(got[:, 0] - ref)
    # and far closer than the in-sample lpd is: the held-out correction matters most for the outlying observation
    lpd = got[:, 0] + got[:, 1]
    assert abs(lpd[0] - ref[0]) > 10 * abs(got[0, 0] - ref[0])
    assert np.all(got[:, 1] > 0) and np.allclose(got[:, 2], -2 * got[:, 0], rtol=0, atol=0)


def test_excluded_cell_is_the_held_out_density():
    _, _, ll = _normal_mean_problem(n_draws=2000, seed=1)
    lpd = math.log(np.mean(np.exp(ll[:, 3])))
    e, p, ic, k = L.loo_point(ll[:, 3], excluded=True)
    assert abs(e - lpd) < 1e-12 and p == 0.0 and ic == -2 * e and np.isnan(k)


@pytest.mark.parametrize("s2", [2.0, 4.0, 10.0])
def test_normal_ratios_recover_the_shape(s2):
    r = L.P.normal_ratios(np.random.default_rng(0), s2, 100_000)
    k = L.loo_point(-r)[3]
    assert abs(k - (1.0 - 1.0 / s2)) <= 0.1, (s2, k)


def test_tail_length_with_r_eff():
    assert L.tail_len(4000) == 190 and L.tail_len(4000, 0.25) == 380 and L.tail_len(4000, 4.0) == 95
    assert L.tail_len(100, 0.01) == 20                          # 0.2 N binds


def test_smoothed_weights_are_truncated_and_monotone():
    r = L.P.normal_ratios(np.random.default_rng(2), 3.0, 4000)
    lw, k = L.psis_log_weights(r)
    assert np.isfinite(k) and lw.max() <= 0.0
    order = np.argsort(r, kind="stable")
    assert np.all(np.diff(lw[order]) >= 0)                      # smoothing keeps the ratios' order


def test_estimates_leave_excluded_cells_out():
    pw = np.array([[-1.0, 0.5, 2.0, 0.1], [-2.0, 0.25, 4.0, 0.2], [-9.0, 0.0, 18.0, np.nan]])
    est = L.estimates(pw, excluded=[False, False, True])
    assert est["elpd_loo"] == (-3.0, math.sqrt(2 * 0.5))
    assert est["p_loo"][0] == 0.75 and est["looic"][0] == 6.0
