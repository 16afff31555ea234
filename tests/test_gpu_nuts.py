"""The device's NUTS warm-up and kept draws against oracle.nuts_model on the qualified cases of tests/nuts_cases.py: the integer
decisions of every iteration identical, step sizes, acceptance, kept draws, lp and the adapted inverse metric (all D entries; the
six hyper coordinates, which live in a copy of their own, named apart) within 10 times the case's yardstick for that quantity
("How NUTS is held") -- in both round structures, at 1 and 64 lanes per gene, in one and two chain groups."""
import numpy as np
import pytest

from tests import nuts_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from ppcseq_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the product has no CPU fallback")
    return _lib


@pytest.fixture(scope="module")
def yardsticks():
    """name -> the case's yardsticks; every one <= 1e-6 is asserted here, so no tolerance below exceeds 1e-5"""
    def get(name):
        _, Y, why = NC.qualified(name)
        assert why == [] and max(Y.values()) <= NC.Y_MAX, (name, Y, why)
        return Y
    return get


@pytest.fixture(scope="module")
def references(oracle):
    """name -> oracle.nuts_model of the case, computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = NC.oracle_run(oracle, NC.CASES[name])
        return memo[name]
    return get


def _model(L, case):
    d, excl = case.data()
    return L.Model(d["counts"], d["X"], d["exposure"], case.K, excl=excl)


def _fit(m, case):
    f = m.fit_nuts(chains=case.chains, chain_id_offset=case.chain_id_offset, **case.cfg)
    try:
        return dict(draws=f.draws(), inv_metric=f.inv_metric(), **f.diagnostics())
    finally:
        f.close()


def _follows(case, res, ref, Y, what):
    name, h = case.name, list(case.hyper)
    d = NC.differences(res, ref)
    hyp = float(np.max(np.abs(res["inv_metric"][:, h] - ref["inv_metric"][:, h]) / ref["inv_metric"][:, h]))
    print(f"case {name}, {what}: device to oracle " + ", ".join(f"{q} {d[q]:.3g} (Y {Y[q]:.3g})" for q in NC.QUANTITIES)
          + f", inv_metric of the hyper coordinates {hyp:.3g}")
    assert NC.integer_differences(res, ref) == [], (name, what)
    assert hyp <= NC.HOLD * Y["inv_metric"], (name, what, "inverse metric of the hyper coordinates", hyp)
    assert NC.exceeded(res, ref, Y) == {}, (name, what)
    if name == "N6":
        assert np.all(res["stepsize"][:, case.cfg["warmup"]:] == 1.0), (name, what, res["stepsize"][:, case.cfg["warmup"]:])
    if name == "N7":
        assert np.all(res["inv_metric"] == 1.0), (name, what)


@pytest.mark.parametrize("pipelined", [-1, 0])
@pytest.mark.parametrize("name", NC.ROWS)
def test_fit_follows_oracle(L, yardsticks, references, name, pipelined):
    case = NC.CASES[name]
    m = _model(L, case)
    try:
        m.set_rounds(pipelined=pipelined)
        _follows(case, _fit(m, case), references(name), yardsticks(name), f"rounds {'pipelined' if pipelined else 'classic'}")
    finally:
        m.close()


@pytest.mark.parametrize("lanes", [1, 64])
def test_three_workgroups_at_one_and_64_lanes_per_gene(L, yardsticks, references, lanes):
    case = NC.CASES["N5"]
    m = _model(L, case)
    try:
        m.set_launch(lanes, 0)
        _follows(case, _fit(m, case), references("N5"), yardsticks("N5"), f"{lanes} lanes per gene")
    finally:
        m.close()


def test_five_chains_in_two_groups_and_in_one(L, yardsticks, references):
    """N1's five chains run as two chain groups by default; as one group they are the same chains bit for bit"""
    case = NC.CASES["N1"]
    m = _model(L, case)
    try:
        assert m.get_rounds(case.chains)[1] == 2
        two = _fit(m, case)
        m.set_rounds(stream_groups=1)
        assert m.get_rounds(case.chains)[1] == 1
        one = _fit(m, case)
    finally:
        m.close()
    _follows(case, two, references("N1"), yardsticks("N1"), "two chain groups")
    _follows(case, one, references("N1"), yardsticks("N1"), "one chain group")
    for k in NC.QUANTITIES + NC.INTEGERS:
        assert np.array_equal(one[k], two[k]), k
