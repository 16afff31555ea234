"""The device's ADVI (ppcx_fit_advi, ppcx_fit_advi_iterative) step for step against oracle.advi on the qualified cases of
tests/advi_cases.py: short runs over the designs, launch shapes and branches of the fit, held to 10 Y, where Y <= 1e-8 is what
gradient errors of the size the suite allows the device move the case (DESIGN.md "ADVI"). Then what no amplification touches: the
draw ids of the output rows, the retry wrapper, refusals, determinism."""
import ctypes as C

import numpy as np
import pytest

from tests import advi_cases as AC
from tests import advi_restate as R

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STEPSIZE, ERR_LIMIT = -1, -4, -6    # include/ppcx.h


@pytest.fixture(scope="module")
def L():
    from ppcseq_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the product has no CPU fallback")
    return _lib


@pytest.fixture(scope="module")
def yardstick():
    """name -> (the restatement's result, Y); Y <= 1e-8 is asserted here, so no tolerance below exceeds 1e-7"""
    def get(name):
        base, Y, why = AC.qualified(name)
        assert why == [] and Y <= AC.Y_MAX, (name, Y, why)
        return base, Y
    return get


@pytest.fixture(scope="module")
def references(oracle):
    """name -> oracle.advi of the case, computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            case = AC.CASES[name]
            d, excl = case.data()
            mo = oracle.model(d["counts"], d["X"], d["exposure"], case.K, excl=excl)
            memo[name] = oracle.advi(mo, **case.full_cfg())
        return memo[name]
    return get


def _model(L, case):
    d, excl = case.data()
    return L.Model(d["counts"], d["X"], d["exposure"], case.K, excl=excl)


def _result(f):
    mu, om = f.approximation()
    return dict(mu=mu, omega=om, draws=f.draws()[0], **f.advi_info())


def _same_bits(a, b):
    return (np.array_equal(a["mu"], b["mu"]) and np.array_equal(a["omega"], b["omega"]) and np.array_equal(a["draws"], b["draws"])
            and all(a[k] == b[k] for k in ("eta", "iterations", "converged", "elbo")))


def _follows(name, res, ro, Y, what=""):
    assert (res["eta"], res["iterations"], bool(res["converged"])) == (ro["eta"], ro["iterations"], ro["converged"]), (name, what)
    dist = AC.distance(res, ro)
    print(f"case {name}{what}: device to oracle {dist:.3g} (mu {np.max(np.abs(res['mu'] - ro['mu'])):.3g}, omega "
          f"{np.max(np.abs(res['omega'] - ro['omega'])):.3g}, draws {np.max(np.abs(res['draws'] - ro['draws'])):.3g}, elbo "
          f"{abs((res['elbo'] - ro['elbo']) / ro['elbo']):.3g}), Y = {Y:.3g}")
    assert np.max(np.abs(res["mu"] - ro["mu"])) <= 10 * Y, (name, what)
    assert np.max(np.abs(res["omega"] - ro["omega"])) <= 10 * Y, (name, what)
    assert np.max(np.abs(res["draws"] - ro["draws"])) <= 10 * Y, (name, what)
    assert abs((res["elbo"] - ro["elbo"]) / ro["elbo"]) <= 10 * Y, (name, what)


@pytest.mark.parametrize("name", AC.FITTED)
def test_fit_follows_oracle(L, yardstick, references, name):
    case = AC.CASES[name]
    _, Y = yardstick(name)
    ro = references(name)
    m = _model(L, case)
    try:
        for lanes in ((None, 0, 1, 64) if name == "D" else (None,)):   # D: the log-likelihood's reductions, too
            if lanes is not None:
                m.set_launch(lanes, 0)
            f = m.fit_advi(**case.full_cfg())
            try:
                _follows(name, _result(f), ro, Y, "" if lanes is None else f", {lanes} lanes per gene")
            finally:
                f.close()
    finally:
        m.close()


@pytest.mark.parametrize("name", ["B", "D"])
def test_output_rows_take_their_draw_ids(L, yardstick, name):
    """Row r of the fit is mu + exp(omega) eta(first output id + r) on the device's own mu and omega, the normals from the
    restatement's Philox: the order ELBO batches -> gradient draws -> output rows of 64. 1e-12 (|mu| + e^omega (1 + |eta|)) is a
    thousand roundings of the operations involved, and orders below what a wrong draw id or row offset gives."""
    case = AC.CASES[name]
    base, _ = yardstick(name)
    cfg = case.full_cfg()
    m = _model(L, case)
    try:
        f = m.fit_advi(**cfg)
        try:
            res = _result(f)
        finally:
            f.close()
    finally:
        m.close()
    assert (res["eta"], res["iterations"]) == (base["eta"], base["iterations"])
    assert res["draws"].shape == (cfg["output_samples"], case.D)
    sd = np.exp(res["omega"])
    for r in range(cfg["output_samples"]):
        eta = R.eta_draw(case.D, base["first_output_id"] + r, R.seed32(cfg["seed"]))
        tol = 1e-12 * (np.abs(res["mu"]) + sd * (1 + np.abs(eta)))
        assert np.all(np.abs(res["draws"][r] - (res["mu"] + sd * eta)) <= tol), (name, r)


def test_every_step_size_fails_once_then_retries(L):
    """Case H. One attempt: PPCX_ERR_STEPSIZE, and nothing stays allocated. Two attempts: the fit of seed + 1, bit for bit (device
    against device: seed 8 is ill-conditioned against the oracle)."""
    case = AC.CASES["H"]
    cfg = case.full_cfg()
    assert cfg["seed"] == 7 and AC.qualified("H")[0] is None and AC.qualified("H")[2] == []
    m = _model(L, case)
    try:
        with pytest.raises(L.PpcxError, match=f"ppcx error {ERR_STEPSIZE}:"):    # (also: nothing is left to load lazily below)
            m.fit_advi(**cfg)
        before = L.device_memory()
        with pytest.raises(L.PpcxError, match=f"ppcx error {ERR_STEPSIZE}:"):
            m.fit_advi(**cfg, max_attempts=1)
        assert L.device_memory() == before
        f2 = m.fit_advi(**cfg, max_attempts=2)
        f8 = m.fit_advi(**dict(cfg, seed=8), max_attempts=1)
        try:
            assert _same_bits(_result(f2), _result(f8))
        finally:
            f2.close(); f8.close()
    finally:
        m.close()


def test_refusals(L):
    case = AC.CASES["A"]
    m = _model(L, case)
    try:
        for bad in ("output_samples", "iter", "elbo_samples", "eval_elbo", "adapt_iter", "tol_rel_obj"):
            for attempts in (1, 3):              # the plain entry and the retry wrapper
                with pytest.raises(L.PpcxError, match=f"ppcx error {ERR_ARG}:"):
                    m.fit_advi(**dict(case.full_cfg(), **{bad: 0}), max_attempts=attempts)
        c = case.full_cfg()
        for grad_samples, bad, rc in ((2, {}, ERR_LIMIT), (1, dict(iter=0), ERR_ARG), (1, dict(tol_rel_obj=0.0), ERR_ARG)):
            c1 = dict(c, **bad)
            cfg = L.AdviConfig(c1["output_samples"], c1["iter"], c1["tol_rel_obj"], grad_samples, c1["elbo_samples"], c1["eval_elbo"],
                               c1["adapt_iter"], c1["seed"], 2.0)
            for call in (lambda h: L.load().ppcx_fit_advi(m._h, C.byref(cfg), C.byref(h)),
                         lambda h: L.load().ppcx_fit_advi_iterative(m._h, C.byref(cfg), 2, C.byref(h))):
                h = C.c_void_p(0xdead)           # the entry clears the handle it refuses to fill
                assert call(h) == rc and not h.value
    finally:
        m.close()


def test_fit_is_deterministic(L):
    case = AC.CASES["D"]
    m = _model(L, case)
    try:
        fits = [m.fit_advi(**case.full_cfg()) for _ in range(2)]
        try:
            assert _same_bits(_result(fits[0]), _result(fits[1]))
        finally:
            for f in fits:
                f.close()
    finally:
        m.close()
