"""NUTS warm-up and kept draws held to an independent restatement (tests/nuts_restate.py) on the qualified short cases of
tests/nuts_cases.py ("How NUTS is held"): the restatement against the oracle and against a Gaussian's known
answers, the host emulation of the device's state machine (classic and pipelined rounds) against the oracle to the same bounds,
and the proof that the bounds bite: each seeded fault moves at least one row past them."""
import numpy as np
import pytest

from tests import nuts_cases as NC
from tests import nuts_restate as R
from tests.emul_util import emul_fit, emul_fit_pipelined

# The yardsticks as measured (DESIGN.md section 4 carries the same table): a case that drifts is noticed here.
YARDSTICKS = {
    "N1": dict(draws=3.8e-07, lp=7.4e-09, stepsize=1.0e-07, accept=6.7e-08, inv_metric=2.5e-07),
    "N2": dict(draws=9.4e-08, lp=2.7e-10, stepsize=3.1e-08, accept=3.0e-07, inv_metric=5.8e-09),
    "N3": dict(draws=3.7e-08, lp=2.2e-09, stepsize=1.9e-08, accept=5.1e-09, inv_metric=1.3e-08),
    "N4": dict(draws=2.7e-08, lp=2.6e-10, stepsize=1.2e-08, accept=3.2e-09, inv_metric=1.0e-08),
    "N5": dict(draws=4.8e-08, lp=3.1e-10, stepsize=7.5e-09, accept=2.5e-08, inv_metric=8.6e-09),
    "N6": dict(draws=5.3e-08, lp=3.8e-09, stepsize=2.4e-08, accept=1.3e-08, inv_metric=2.6e-08),
    "N7": dict(draws=2.2e-09, lp=5.7e-11, stepsize=2.1e-10, accept=1.6e-09, inv_metric=0.0),
    "N8": dict(draws=1.1e-08, lp=1.5e-10, stepsize=2.8e-08, accept=1.4e-08, inv_metric=5.8e-09),
}

# Which rows each seeded fault moves past its bounds against the oracle (measured; at least these must fail). N7 has no windowed
# adaptation and only sees what touches dual averaging before the first update.
FAULT_ROWS = {
    "welford_n": ("N1", "N2", "N3", "N4", "N5", "N6", "N8"),
    "regulariser": ("N1", "N2", "N3", "N4", "N5", "N6", "N8"),
    "set_mu": ("N1", "N2", "N3", "N4", "N5", "N6", "N7", "N8"),
    "no_restart": ("N1", "N2", "N3", "N4", "N5", "N6", "N8"),
    "eps_call": ("N1", "N3", "N4", "N5", "N8"),  # N2, N6: the search ends at the same power of two under call 0's momenta
    "no_doubling": ("N3", "N4", "N6"),           # N2: the undoubled window is stretched to the same end, 18
    "hyper_unit": ("N1", "N2", "N3", "N4", "N5", "N6", "N8"),
    "no_complete": ("N1", "N2", "N4", "N5", "N6", "N7", "N8"),   # N3: one iteration after the restart, x_bar = x
}


@pytest.fixture(scope="module")
def references(oracle):
    """name -> oracle.nuts_model of the case in the common form, computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = NC.oracle_run(oracle, NC.CASES[name])
        return memo[name]
    return get


def _qualified(name):
    base, Y, why = NC.qualified(name)
    assert why == [] and max(Y.values()) <= NC.Y_MAX, (name, Y, why)
    return base, Y


def _follows(name, res, ref, Y, what):
    d = NC.differences(res, ref)
    print(f"case {name}, {what}: " + ", ".join(f"{q} {d[q]:.3g} (Y {Y[q]:.3g})" for q in NC.QUANTITIES))
    assert NC.integer_differences(res, ref) == [], (name, what)
    assert NC.exceeded(res, ref, Y) == {}, (name, what)


def test_every_row_has_a_case():
    assert NC.ROWS == tuple(f"N{k}" for k in range(1, 9)) and set(YARDSTICKS) == set(NC.ROWS)


@pytest.mark.parametrize("name", NC.ROWS)
def test_case_qualifies(name):
    """The integer decisions hold under the ten perturbed runs, every yardstick is at most 1e-6 and is the one the table states,
    and the metric is updated at the iterations the schedule gives by hand, from the number of draws it gives."""
    case = NC.CASES[name]
    base, Y = _qualified(name)
    print(f"case {name}: " + ", ".join(f"Y[{q}] = {Y[q]:.2g}" for q in NC.QUANTITIES))
    for q in NC.QUANTITIES:
        pin = YARDSTICKS[name][q]
        assert (Y[q] == 0.0) if pin == 0.0 else abs(Y[q] / pin - 1.0) <= 0.25, (name, q, Y[q], pin)
    assert base["updates"] == [list(case.updates)] * case.chains
    for hist in base["metric_history"]:
        assert all(np.all(np.isfinite(m)) and np.all(m > 0) for _, _, m in hist)
    if name == "N6":
        assert np.all(base["stepsize"][:, case.cfg["warmup"]:] == 1.0)
    if name == "N7":
        assert np.all(base["inv_metric"] == 1.0)


def test_cases_keep_the_branches_they_were_chosen_for():
    """Divergent transitions, trees that reach max_treedepth, and a start that needs a second init attempt"""
    for name in NC.ROWS:
        base, _ = _qualified(name)
        assert base["divergent"].sum() >= 2 and (base["treedepth"] == NC.CASES[name].cfg["max_treedepth"]).sum() >= 2, name
    assert _qualified("N2")[0]["init_attempts"] == [2, 1]


@pytest.mark.parametrize("name", NC.ROWS)
def test_restatement_follows_oracle(references, name):
    base, Y = _qualified(name)
    _follows(name, base, references(name), Y, "restatement to oracle")


def test_restatement_on_a_gaussian():
    """A short version of test_oracle_nuts.test_adaptation_schedule on N(0, 0.01^2 I), D = 10, windows 10 / 10 / 10 of a warm-up of
    30: one update at iteration 19 from 10 draws; before it the step size is of the target's scale (the leapfrog is unstable beyond
    2 sd = 0.02), after it of the unit scale; the metric is the regularised variance of 10 draws of variance 1e-4 (chi-square with
    9 degrees of freedom: within a factor 0.1 .. 4 of it); lp of a kept draw is the density at the draw; the kept step size is
    exp(x_bar) recomputed from the acceptance trace since the restart."""
    D, sd = 10, 0.01

    def density(u):
        z = u / sd
        return -0.5 * float(np.dot(z, z)), -z / sd
    r = R.nuts_chain(density, D, iter=36, warmup=30, seed=3, init_buffer=10, window=10, term_buffer=10)
    assert [(it, n) for it, n, _ in r.metric_updates] == [(19, 10)]
    assert r.stepsize[12:20].max() < 0.03 and r.stepsize[21:].min() > 0.05
    var = (r.inv_metric - 1e-3 * 5.0 / 15.0) * 15.0 / 10.0
    assert np.all(var > 0.1 * sd * sd) and np.all(var < 4.0 * sd * sd)
    assert np.allclose(r.lp, -0.5 * np.sum((r.draws / sd) ** 2, axis=1), rtol=1e-12)
    assert r.divergent[30:].sum() == 0 and np.all(r.stepsize[30:] == r.stepsize[30])
    mu, s_bar, x_bar = np.log(10.0 * r.stepsize[20]), 0.0, 0.0
    for t in range(1, 11):
        s_bar += (0.8 - min(r.accept[19 + t], 1.0) - s_bar) / (t + 10.0)
        x = mu - s_bar * np.sqrt(t) / 0.05
        x_bar += (x - x_bar) * t ** -0.75
        if t < 10:
            assert abs(r.stepsize[20 + t] / np.exp(x) - 1.0) < 1e-12
    assert abs(r.stepsize[30] / np.exp(x_bar) - 1.0) < 1e-12


def _emul_args(case):
    d, excl = case.data()
    c = case.cfg
    kw = {k: c[k] for k in ("init_buffer", "term_buffer", "window") if k in c}
    return (d["counts"], d["X"], d["exposure"], case.K, case.chains, c["iter"], c["warmup"], c["seed"]), dict(
        excl=excl, max_treedepth=c["max_treedepth"], chain_id_offset=case.chain_id_offset, **kw)


@pytest.mark.parametrize("name", NC.ROWS)
def test_emulation_follows_oracle(emul, references, name):
    """The device's state machine and per-coordinate updates on the host, classic rounds: Welford, the metric of gene and hyper
    coordinates, the restarted search and dual averaging, complete_adaptation, kept draws"""
    _, Y = _qualified(name)
    a, kw = _emul_args(NC.CASES[name])
    _follows(name, emul_fit(emul, *a, **kw), references(name), Y, "emulation to oracle")


@pytest.mark.parametrize("name", NC.ROWS)
def test_pipelined_emulation_follows_oracle(emul, references, name):
    """The two-launch rounds, with and without anticipated positions and in both launch orders"""
    _, Y = _qualified(name)
    a, kw = _emul_args(NC.CASES[name])
    for spec in (True, False):
        for ls_first_s in (False, True):
            e = emul_fit_pipelined(emul, *a, spec=spec, ls_first_s=ls_first_s, **kw)
            _follows(name, e, references(name), Y, f"pipelined emulation (spec {spec}, state machine first {ls_first_s}) to oracle")


@pytest.mark.parametrize("fault", R.FAULTS)
def test_seeded_fault_is_caught(oracle, references, fault):
    """Each silent mistake, seeded in the restatement, moves the rows of FAULT_ROWS past the bounds the comparisons hold"""
    failing = []
    for name in NC.ROWS:
        case = NC.CASES[name]
        _, Y = _qualified(name)
        r = NC.run(case, NC.oracle_density(oracle, case), faults=(fault,))
        if NC.integer_differences(r, references(name)) or NC.exceeded(r, references(name), Y):
            failing.append(name)
    print(f"fault {fault}: rows {failing}")
    assert failing and set(FAULT_ROWS[fault]) <= set(failing), (fault, failing)
