"""The streamed route of the log-likelihood kernel (Model(per_sample="stream" | "auto"); include/ppcx.h ppcx_model_create_ex): the
per-sample constants read from global memory instead of LDS, for designs whose S * C doubles do not fit LDS beside the tables.

Tolerances are those of tests/test_gpu_parity.py: |lp - lp_o| <= 1e-11 max(1, |lp_o|), max |g - g_o| / (1 + |g_o|) <= 1e-10 against
the oracle; between the two routes of one model lp within 1e-13 relative (the bound test_continuous_covariate_and_two_group_designs
puts between two routes of one model) and the gradient in the 1e-10 form. The sampler and ADVI are held by their cases' own criteria
(tests/nuts_cases.py, tests/advi_cases.py)."""
import numpy as np
import pytest

from oracle import independent as ind
from tests import advi_cases as AC
from tests import nuts_cases as NC
from tests import test_gpu_advi as TA
from tests import test_gpu_nuts as TN

pytestmark = pytest.mark.gpu

ERR_LIMIT = -6                                   # include/ppcx.h
LDS_DOUBLES = 17408                              # per-sample constants that fit LDS: (160 KB - 20 KB of tables - 2 pads of 256) / 8


@pytest.fixture(scope="module")
def L():
    from ppcseq_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the product has no CPU fallback")
    return _lib


def _two_groups(G, S, K, seed):
    d = ind.synth(G, S, K=K, seed=seed, C=2)
    return d["counts"], d["X"], d["exposure"]


def _factor(G, S, K, levels, seed):
    d = ind.synth_factor(G, S, K, levels, seed)
    return d["counts"], d["X"], d["exposure"]


def _continuous_last(G, S, K, levels, seed):
    counts, X, expo = _factor(G, S, K, levels, seed)
    X = X.copy()
    X[:, -1] = np.linspace(-1, 1, S)
    return counts, X, expo


def _no_ones(G, S, K, seed):
    counts, X, expo = _two_groups(G, S, K, seed)
    X = X.copy()
    X[:, 0] = np.linspace(0.5, 1.5, S)
    return counts, X, expo


# name -> (data, K, seed, doubles of per-sample constants: S * C, S * (2 + C) without the column of ones)
OVER_LIMIT = {
    "two groups, S 9216": (lambda: _two_groups(16, 9216, 5, 3), 5, 3, 18432),
    "two groups, S 18432": (lambda: _two_groups(8, 18432, 3, 4), 3, 4, 36864),
    "C 16": (lambda: _factor(24, 1280, 6, (16,), 5), 6, 5, 20480),
    "C 8": (lambda: _factor(24, 2304, 6, (5, 4), 6), 6, 6, 18432),
    "continuous column": (lambda: _continuous_last(20, 6144, 5, (3,), 7), 5, 7, 18432),
    "no column of ones": (lambda: _no_ones(12, 4608, 4, 8), 4, 8, 18432),
}
FIRST = "two groups, S 9216"


def _u(G, C, K, seed, oracle, n=2):
    """the points of test_gpu_parity._point"""
    u = np.random.default_rng(seed).uniform(-1, 1, (n, oracle.dim(G, C, K)))
    u[:, 3:3 + G] += 5
    return u


def _excl(G, S):
    """the exclusion triple of test_gpu_parity._point"""
    return np.array(sorted({1 % (G * S), (2 * S + 3) % (G * S), (G - 1) * S}), dtype=np.int32)


@pytest.fixture(scope="module")
def over_limit(oracle):
    """(name, excluded) -> (counts, X, exposure, K, excl, u, [(lp, grad) of the oracle at u]), computed once and left unchanged"""
    memo = {}

    def get(name, excluded):
        if (name, excluded) not in memo:
            make, K, seed, doubles = OVER_LIMIT[name]
            counts, X, expo = make()
            G, S = counts.shape
            C = X.shape[1]
            assert doubles == S * (C if np.all(X[:, 0] == 1.0) else 2 + C) and doubles > LDS_DOUBLES
            excl = _excl(G, S) if excluded else None
            u = _u(G, C, K, seed, oracle)
            mo = oracle.model(counts, X, expo, K, excl=excl)
            ref = [oracle.log_prob_grad(mo, u[i]) for i in range(u.shape[0])]
            assert all(np.isfinite(r[0]) and np.all(np.isfinite(r[1])) for r in ref)
            memo[(name, excluded)] = (counts, X, expo, K, excl, u, ref)
        return memo[(name, excluded)]
    return get


def _holds(lp, g, ref, what):
    for i, (lpo, go) in enumerate(ref):
        err_lp, err_g = abs(lp[i] - lpo) / max(1.0, abs(lpo)), np.max(np.abs(g[i] - go) / (1 + np.abs(go)))
        print(f"{what}, point {i}: lp {err_lp:.3g}, gradient {err_g:.3g}")
        assert err_lp <= 1e-11, (what, i, lp[i], lpo)
        assert err_g <= 1e-10, (what, i)


@pytest.mark.parametrize("excluded", [False, True])
@pytest.mark.parametrize("name", list(OVER_LIMIT))
def test_over_limit_shapes_match_oracle(L, over_limit, name, excluded):
    """a. Designs past the 17 408 doubles of LDS: refused by default, streamed by "auto", density and gradient against the oracle at
    the automatic lanes per gene and at 1, 8 and 64, with and without excluded cells (the masked sweep)."""
    counts, X, expo, K, excl, u, ref = over_limit(name, excluded)
    with pytest.raises(L.PpcxError, match="LDS"):
        L.Model(counts, X, expo, K, excl=excl)
    m = L.Model(counts, X, expo, K, excl=excl, per_sample="auto")
    try:
        assert m.per_sample == "stream"
        for lanes in (0, 1, 8, 64):
            m.set_launch(lanes, 0)
            lp, g = m.log_prob_grad(u)
            _holds(lp, g, ref, f"{name}, {lanes} lanes per gene")
    finally:
        m.close()


def _design(kind, S, K, seed):
    if kind == "two groups":
        return _two_groups(9, S, K, seed)
    if kind == "three-level factor":
        return _factor(9, S, K, (3,), seed)
    counts, X, expo = _two_groups(9, S, K, seed)
    X = X.copy()
    if kind == "continuous column":
        X[:, 1] = np.linspace(-1.0, 1.5, S)
    else:
        X[:, 0] = np.linspace(0.5, 1.5, S)
    return counts, X, expo


@pytest.mark.parametrize("kind", ["two groups", "three-level factor", "continuous column", "no column of ones"])
@pytest.mark.parametrize("S", [1, 3, 9, 32, 33, 257])
def test_streamed_and_lds_routes_agree(L, oracle, S, kind):
    """b. Where both routes run -- at the sample counts at which the sweep's tail and the pad past the arrays can go wrong, every lane
    count, with and without checked genes and excluded cells: the same numbers, and both the oracle's."""
    G, same_bits, n = 9, 0, 0
    for K in (0, 4):
        counts, X, expo = _design(kind, S, K, 20 + S)
        u = _u(G, X.shape[1], K, S, oracle)
        for excl in (None, _excl(G, S)):
            mo = oracle.model(counts, X, expo, K, excl=excl)
            ref = [oracle.log_prob_grad(mo, u[i]) for i in range(2)]
            res = {}
            for route in ("lds", "stream"):
                m = L.Model(counts, X, expo, K, excl=excl, per_sample=route)
                try:
                    assert m.per_sample == route
                    for lanes in (1, 2, 4, 8, 16, 32, 64):
                        m.set_launch(lanes, 0)
                        res[route, lanes] = m.log_prob_grad(u)
                finally:
                    m.close()
            for lanes in (1, 2, 4, 8, 16, 32, 64):
                (lp_l, g_l), (lp_s, g_s) = res["lds", lanes], res["stream", lanes]
                what = f"S {S}, {kind}, K {K}, {'excluded cells' if excl is not None else 'all cells'}, {lanes} lanes"
                assert np.max(np.abs(lp_s - lp_l) / np.abs(lp_l)) <= 1e-13, what
                assert np.max(np.abs(g_s - g_l) / (1 + np.abs(g_l))) <= 1e-10, what
                _holds(lp_l, g_l, ref, what + ", lds")
                _holds(lp_s, g_s, ref, what + ", stream")
                same_bits += int(np.array_equal(lp_l, lp_s) and np.array_equal(g_l, g_s))
                n += 1
    print(f"S {S}, {kind}: {same_bits} of {n} launches with equal bits on the two routes")


def _three_launch_rounds(m, chains):
    assert m.get_rounds(chains)[0] is False
    m.set_rounds(pipelined=1)
    assert m.get_rounds(chains)[0] is False


def test_sampler_follows_oracle_on_streamed_model(L, oracle):
    """c. N5 of tests/nuts_cases.py by its own criteria, on a streamed model; the model runs the three-launch round whatever is set"""
    case = NC.CASES["N5"]
    _, Y, why = NC.qualified("N5")
    assert why == [] and max(Y.values()) <= NC.Y_MAX
    d, excl = case.data()
    m = L.Model(d["counts"], d["X"], d["exposure"], case.K, excl=excl, per_sample="stream")
    try:
        assert m.per_sample == "stream"
        _three_launch_rounds(m, case.chains)
        TN._follows(case, TN._fit(m, case), NC.oracle_run(oracle, case), Y, "streamed")
    finally:
        m.close()


def test_advi_follows_oracle_on_streamed_model(L, oracle):
    """c. D of tests/advi_cases.py by its own criteria, on a streamed model"""
    case = AC.CASES["D"]
    _, Y, why = AC.qualified("D")
    assert why == [] and Y <= AC.Y_MAX
    d, excl = case.data()
    ro = oracle.advi(oracle.model(d["counts"], d["X"], d["exposure"], case.K, excl=excl), **case.full_cfg())
    m = L.Model(d["counts"], d["X"], d["exposure"], case.K, excl=excl, per_sample="stream")
    try:
        f = m.fit_advi(**case.full_cfg())
        try:
            TA._follows("D", TA._result(f), ro, Y, ", streamed")
        finally:
            f.close()
    finally:
        m.close()


def test_short_fit_on_over_limit_shape_follows_oracle(L, oracle, over_limit):
    """c. The first iterations of a fit on a design that only the streamed route accepts, as test_factor_designs_factorise_and_pipeline
    holds them"""
    counts, X, expo, K, _, _, _ = over_limit(FIRST, False)
    r = oracle.nuts_model(oracle.model(counts, X, expo, K), oracle.cfg(chains=2, iter=14, warmup=10, seed=5))
    m = L.Model(counts, X, expo, K, per_sample="auto")
    try:
        _three_launch_rounds(m, 2)
        f = m.fit_nuts(chains=2, iter=14, warmup=10, seed=5)
        dg = f.diagnostics()
        f.close()
    finally:
        m.close()
    assert np.array_equal(dg["n_leapfrog"][:, :6], r.n_leapfrog[:, :6])
    assert np.allclose(dg["stepsize"][:, :6], r.stepsize[:, :6], rtol=1e-9, atol=0)


def test_downstream_of_a_fit_on_over_limit_shape(L, oracle, over_limit):
    """d. What reads a fit's draws per cell does not depend on S in the kernel's way: predictive draws bit for bit, intervals, LOO and
    the exact predictive on a streamed model"""
    counts, X, expo, K, _, _, _ = over_limit(FIRST, False)
    G, S = counts.shape
    draws = _u(G, X.shape[1], K, 31, oracle, n=64).reshape(2, 32, -1)
    mo = oracle.model(counts, X, expo, K)
    m = L.Model(counts, X, expo, K, per_sample="auto")
    try:
        f = m.fit_from_draws(draws)
        try:
            ci, rng = f.ppc(1.0, 0.05, 0.95, seed=5, return_counts_rng=True)
            gq = oracle.generated_quantities(mo, draws.reshape(64, -1), 1.0, seed=5)
            assert np.array_equal(gq, rng)
            assert np.max(np.abs(oracle.summarise(gq, 0.05, 0.95) - ci)) < 1e-9
            loo = f.loo(genes=np.arange(K))
            for k in ("elpd_loo", "p_loo", "looic", "khat"):
                assert loo[k].shape == (K, S) and np.all(np.isfinite(loo[k])), k
            ex = f.ppc_exact()
            for k in ("mean", "sd", "p_le", "p_ge", "lower", "upper"):
                assert ex[k].shape == (K, S) and np.all(np.isfinite(ex[k])), k
        finally:
            f.close()
    finally:
        m.close()


def test_refusals_stay_statuses(L):
    """e. Beyond the dispersion-table kernel's row, and a continuous covariate among more than 8 columns: PPCX_ERR_LIMIT, by message"""
    rng = np.random.default_rng(1)
    S = 40000
    X = np.stack([np.ones(S), (np.arange(S) % 2).astype(float)], axis=1)
    with pytest.raises(L.PpcxError, match=f"ppcx error {ERR_LIMIT}:.*dispersion-table kernel"):
        L.Model(rng.poisson(50.0, (2, S)).astype(np.int32), X, np.zeros(S), 1, per_sample="stream")
    counts, X, expo = _factor(12, 40, 4, (10,), 2)
    X = X.copy()
    X[:, -1] = np.linspace(-1, 1, 40)
    assert X.shape[1] == 10
    with pytest.raises(L.PpcxError, match=f"ppcx error {ERR_LIMIT}:.*more than 8 design columns"):
        L.Model(counts, X, expo, 4, per_sample="auto")


def test_auto_keeps_an_accepted_model_on_lds(L, oracle):
    """"auto" where today's model is accepted is today's model: the LDS route, pipelined rounds, the same bits"""
    counts, X, expo = _two_groups(40, 21, 5, 2)
    u = _u(40, 2, 5, 2, oracle)
    res = {}
    for route in ("lds", "auto"):
        m = L.Model(counts, X, expo, 5, per_sample=route)
        try:
            assert m.per_sample == "lds" and m.get_rounds(3)[0] is True
            res[route] = m.log_prob_grad(u)
        finally:
            m.close()
    assert np.array_equal(res["lds"][0], res["auto"][0]) and np.array_equal(res["lds"][1], res["auto"][1])
