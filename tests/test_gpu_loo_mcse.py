"""The Monte-Carlo standard error of elpd_loo and the PSIS n_eff per observed cell on the MI355X (include/ppcx.h
ppcx_fit_loo_mcse): the kernel on designed columns (testing build) against the numpy restatement
(tests/loo_mcse_restate.py), its calibration on independent columns, a fit against the restatement on its own log-likelihood,
determinism, refusals and do_inference(loo_mcse).

mcse_elpd_loo is compared relative to the restated value itself at tests/loo_mcse_cases.py MCSE_RTOL = 1.65e-13, ten times the
largest difference measured between the CPU build of the header and the restatement on the designed columns."""
import math

import numpy as np
import pytest

from tests import loo_mcse_cases as K
from tests import loo_mcse_restate as R
from tests import loo_restate as L
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import small_fit, testing_lib, testing_library  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- 1. the kernel on designed columns

@pytest.mark.parametrize("which", ["designed", "small"])
def test_kernel_on_designed_columns(testing_lib, which):
    ll, excl, r_eff = K.designed() if which == "designed" else K.small()
    for with_r_eff in (False, True):
        re = r_eff if with_r_eff else None
        got = testing_lib.testing_loo_mcse(ll, excl, re)
        K.compare(got, K.reference(which, with_r_eff), (which, with_r_eff))
        assert np.array_equal(got[:, :4], testing_lib.testing_loo(ll, excl, re), equal_nan=True)   # the flag changes no bit
        n_part = np.sum(ll[:, -1] != np.inf)
        assert got[-1, 5] == n_part * (r_eff[-1] if with_r_eff else 1.0)        # uniform weights: N r_eff exactly
        if which == "designed":
            assert got[8, 4] == 0.0                                              # the constant column
        else:
            assert got[0, 3] == np.inf                                           # M < 5: raw weights


@pytest.mark.parametrize("n", [4096, 4097])
def test_kernel_either_side_of_the_lds_limit(testing_lib, n):
    """n = kPsisLdsDraws keeps the ratios in LDS, n + 1 in the scratch; two columns per batch give the bits of one batch"""
    rng = np.random.default_rng(n)
    ll = np.stack([-L.P.normal_ratios(rng, 2.5, n) for _ in range(4)] + [rng.normal(-4.0, 0.5, size=n)], axis=1)
    excl = np.array([0, 0, 0, 0, 1], np.int32)
    r_eff = rng.uniform(0.4, 1.6, size=5)
    one = testing_lib.testing_loo_mcse(ll, excl, r_eff)
    K.compare(one, R.mcse_columns(ll, r_eff, excl.astype(bool)), ("n", n))
    assert one[4, 5] == n * r_eff[4]
    testing_lib.testing_set("loo_scratch_bytes", 2 * 8 * n + 8)                  # two columns per batch
    try:
        assert np.array_equal(testing_lib.testing_loo_mcse(ll, excl, r_eff), one, equal_nan=True)
    finally:
        testing_lib.testing_set("loo_scratch_bytes", 0)


# ---- 2. calibration

@pytest.mark.parametrize("s", [0.3, 0.8])
def test_calibration(testing_lib, s):
    """200 independent columns of 2 000 independent draws ll ~ Normal(-4, s): the standard deviation of the device's elpd_loo
    across the columns over the median device mcse_elpd_loo lies in [0.8, 1.25], about four standard errors of a standard
    deviation estimated from 200 replicates (1 / sqrt(400) = 5 % each). The restatement alone gives 0.99 (s = 0.3) and 0.95
    (s = 0.8) on exactly these inputs, computed on the CPU."""
    ll = np.random.default_rng(7).normal(-4.0, s, size=(200, 2000)).T
    got = testing_lib.testing_loo_mcse(ll)
    assert np.all(np.isfinite(got[:, [0, 4, 5]])) and np.all(got[:, 4] > 0)
    ratio = float(np.std(got[:, 0], ddof=1) / np.median(got[:, 4]))
    print(f"calibration s={s}: sd(elpd_loo) / median(mcse_elpd_loo) = {ratio:.4f}")
    assert 0.8 <= ratio <= 1.25, ratio
    assert np.all(got[:, 5] <= 2000.0) and np.all(got[:, 5] >= 1.0)


# ---- 3. a fit

def test_fit_matches_restatement(small_fit):
    m, f, d = small_fit
    ll = f.log_lik().reshape(-1, m.G * m.S)
    n = ll.shape[0]
    excl = np.zeros(m.G * m.S, bool)
    excl[[3, 17]] = True
    base = f.loo()
    rng = np.random.default_rng(0)
    for r_eff in (None, rng.uniform(0.2, 1.5, size=(m.G, m.S)), "auto"):
        res = f.loo(r_eff=r_eff, mcse=True)
        plain = base if r_eff is None else f.loo(r_eff=r_eff)
        assert set(res) - set(plain) == {"mcse_elpd_loo", "n_eff", "mcse_elpd_loo_total"}
        for k in L.FIELDS:
            assert np.array_equal(res[k], plain[k], equal_nan=True), k                   # the same bits as ppcx_fit_loo
        re = np.ones(m.G * m.S) if r_eff is None else (res["r_eff"] if isinstance(r_eff, str) else r_eff).ravel()
        ref = R.mcse_columns(ll, re, excl)
        got = np.stack([res[k].ravel() for k in R.FIELDS], axis=1)
        for i in (0, 1, 2, 3, 5):
            fin = np.isfinite(ref[:, i])
            assert np.array_equal(np.isnan(got[:, i]), np.isnan(ref[:, i])), R.FIELDS[i]
            assert np.array_equal(got[~fin & ~np.isnan(ref[:, i]), i], ref[~fin & ~np.isnan(ref[:, i]), i]), R.FIELDS[i]
            err = np.abs(got[fin, i] - ref[fin, i]) / np.maximum(1.0, np.abs(ref[fin, i]))
            assert err.max(initial=0.0) <= 1e-12, (R.FIELDS[i], err.max())
        assert np.all(np.isfinite(ref[:, 4])) and np.all(ref[:, 4] > 0)
        rel = np.abs(got[:, 4] - ref[:, 4]) / ref[:, 4]
        worst = int(np.argmax(rel))
        print(f"fit, r_eff {r_eff if r_eff is None or isinstance(r_eff, str) else 'array'}: largest relative difference of "
              f"mcse_elpd_loo {rel[worst]:.3g} (k-hat {ref[worst, 3]:.3g})")
        assert rel[worst] <= K.MCSE_RTOL, (worst, rel[worst], ref[worst])
        assert np.array_equal(res["n_eff"].ravel()[excl], n * re[excl])                  # excluded: N r_eff exactly
        keep = ~excl
        thr = min(1.0 - 1.0 / math.log10(n), 0.7)
        total = res["mcse_elpd_loo_total"]
        if np.any(res["khat"].ravel()[keep] > thr):
            assert np.isnan(total)
        else:
            assert abs(total - math.sqrt(np.sum(ref[keep, 4] ** 2))) <= 1e-11 * total


def test_fit_determinism_and_subsets(small_fit):
    m, f, d = small_fit
    a, b = f.loo(mcse=True), f.loo(mcse=True)
    sub = np.array([7, 0, 29, 4])
    s = f.loo(sub, mcse=True)
    re = np.random.default_rng(1).uniform(0.3, 1.4, size=(m.G, m.S))
    ar, sr = f.loo(r_eff=re, mcse=True), f.loo(sub, r_eff=re[sub], mcse=True)
    for k in R.FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(s[k], a[k][sub], equal_nan=True), k
        assert np.array_equal(sr[k], ar[k][sub], equal_nan=True), k


def test_fit_batches_give_the_same_bits(small_fit):
    m, f, d = small_fit
    base, dr = f.loo(mcse=True), f.draws()
    with testing_library() as _lib:
        mt = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=np.array([3, 17], np.int32), device=0)
        try:
            ft = mt.fit_from_draws(dr)
            try:
                _lib.testing_set("loo_scratch_bytes", 2 * 8 * 1000 + 8)      # the gene table in batches of one or two genes
                try:
                    got = ft.loo(mcse=True)
                finally:
                    _lib.testing_set("loo_scratch_bytes", 0)
            finally:
                ft.close()
        finally:
            mt.close()
    for k in R.FIELDS:
        assert np.array_equal(got[k], base[k], equal_nan=True), k


# ---- 4. refusals

def test_refusals(small_fit):
    from ppcseq_amd import _lib
    m, f, d = small_fit
    for bad in ([m.G], [-1]):
        with pytest.raises(_lib.PpcxError, match="gene out of range"):
            f.loo(bad, mcse=True)
    for r in (0.0, -1.0, np.nan, np.inf):
        re = np.ones((2, m.S)); re[1, 3] = r
        with pytest.raises(_lib.PpcxError, match="r_eff"):
            f.loo([0, 1], r_eff=re, mcse=True)
    with pytest.raises(ValueError, match="r_eff"):
        f.loo(r_eff="bogus", mcse=True)
    a = m.fit_advi(output_samples=100, iter=500, seed=1)
    try:
        with pytest.raises(_lib.PpcxError, match="NUTS"):
            a.loo(mcse=True)
    finally:
        a.close()


# ---- 5. do_inference

def test_do_inference_loo_mcse(bundled):
    from ppcseq_amd.inference import do_inference, pareto_k_table
    counts, X, _, Kc = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    kw = dict(how_many_posterior_draws=400, cores=4, seed=11, check_loo=True)
    plain = do_inference(counts, X, libsize.mean() - libsize, Kc, **kw)
    res = do_inference(counts, X, libsize.mean() - libsize, Kc, loo_mcse=True, **kw)
    assert set(plain.loo) == {"elpd_loo", "p_loo", "looic", "khat", "excluded", "genes", "n_draws", "estimates"}
    assert set(res.loo) == set(plain.loo) | {"mcse_elpd_loo", "n_eff", "mcse_elpd_loo_total"}
    S = counts.shape[1]
    for k in L.FIELDS:
        assert np.array_equal(res.loo[k], plain.loo[k], equal_nan=True), k
    for k in ("mcse_elpd_loo", "n_eff"):
        assert res.loo[k].shape == (Kc, S) and np.all(np.isfinite(res.loo[k])) and np.all(res.loo[k] > 0), k
    assert np.all(res.loo["n_eff"] <= res.loo["n_draws"])
    t = pareto_k_table(res.loo)
    assert sum(b["count"] for b in t["bins"]) == Kc * S
    assert min(b["min_n_eff"] for b in t["bins"] if b["count"]) == res.loo["n_eff"].min()
