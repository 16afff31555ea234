"""The designed log-likelihood columns of the MCSE / n_eff tests, shared by tests/test_loo_mcse_host.py (CPU build of the header)
and tests/test_gpu_loo_mcse.py (the kernel), with their restated fields computed once: the columns of
tests/test_gpu_loo.py::test_kernel_on_designed_columns (normal ratios, a GPD tail, ties, +-Inf, NaN, constant, excluded), and
n = 20 (M = 4: khat = +Inf and raw weights), each with and without r_eff."""
import functools

import numpy as np

from tests import loo_mcse_restate as R
from tests import loo_restate as L

# The bound on |mcse_elpd_loo - restated| / restated. Measured on these columns between the CPU build of ppcx_loo.h and the
# restatement: 1.65e-14 at most (the column of ties with r_eff; the normal ratios of variance 10 give 9e-15, the others below
# 3e-15 -- the weights of the two differ by what their tail fits differ by, and mcse ~ c carries that). The bound is ten times
# the measured value, for the CPU build and for the kernel alike: the kernel composes the same blocks and differs from the CPU
# build in the order of its sums.
MCSE_MEASURED = 1.65e-14
MCSE_RTOL = 10 * MCSE_MEASURED


@functools.lru_cache(maxsize=None)
def designed():
    """(ll [3000, 10], excluded [10] int32, r_eff [10])"""
    rng = np.random.default_rng(4)
    cols = [-L.P.normal_ratios(rng, s2, 3000) for s2 in (1.5, 3.0, 10.0)]
    cols.append(-np.log(L.P.gpd_sample(rng, 0.8, 3000)))
    cols.append(-rng.poisson(3.0, size=3000).astype(float))            # ties in the tail and at the cutoff
    c = rng.normal(size=3000); c[::9] = np.inf; cols.append(c)         # ll = +Inf takes no part
    c = rng.normal(size=3000); c[4] = -np.inf; cols.append(c)          # ll = -Inf: NaN
    c = rng.normal(size=3000); c[8] = np.nan; cols.append(c)
    cols.append(np.full(3000, -2.5))                                   # constant
    cols.append(rng.normal(-4.0, 0.5, size=3000))                      # excluded below
    ll = np.stack(cols, axis=1)
    excl = np.zeros(ll.shape[1], np.int32); excl[-1] = 1
    r_eff = rng.uniform(0.3, 2.0, size=ll.shape[1])
    ll.setflags(write=False); excl.setflags(write=False); r_eff.setflags(write=False)
    return ll, excl, r_eff


@functools.lru_cache(maxsize=None)
def small():
    """ll [20, 2]: M = 4 at r_eff = 1, the second column excluded"""
    ll = np.random.default_rng(12).normal(-3.0, 1.0, size=(20, 2))
    ll.setflags(write=False)
    return ll, np.array([0, 1], np.int32), np.array([0.6, 1.7])


@functools.lru_cache(maxsize=None)
def reference(which, with_r_eff):
    ll, excl, r_eff = designed() if which == "designed" else small()
    ref = R.mcse_columns(ll, r_eff if with_r_eff else None, excl.astype(bool))
    ref.setflags(write=False)
    return ref


def compare(got, ref, what):
    """The first four fields and n_eff by the suite's convention at 1e-12 (NaN and +-Inf in the same places, the rest within
    1e-12 max(1, |ref|)); mcse_elpd_loo relative to the restated value itself at MCSE_RTOL, 0 where that is 0. Returns the
    largest relative difference of mcse_elpd_loo."""
    got, ref = np.asarray(got), np.asarray(ref)
    for i in (0, 1, 2, 3, 5):
        g, r = got[:, i], ref[:, i]
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, R.FIELDS[i])
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), (what, R.FIELDS[i])
        err = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        assert err.max(initial=0.0) <= 1e-12, (what, R.FIELDS[i], err.max())
    g, r = got[:, 4], ref[:, 4]
    assert np.array_equal(np.isnan(g), np.isnan(r)), (what, "mcse_elpd_loo")
    ok = ~np.isnan(r)
    assert np.all(np.isfinite(r[ok])) and np.all(r[ok] >= 0), what
    zero = ok & (r == 0)
    assert np.all(g[zero] == 0), (what, "mcse_elpd_loo where the restated value is 0", g[zero])
    pos = ok & ~zero
    rel = np.abs(g[pos] - r[pos]) / r[pos]
    worst = float(rel.max(initial=0.0))
    print(f"{what}: largest relative difference of mcse_elpd_loo {worst:.3g}")
    assert worst <= MCSE_RTOL, (what, "mcse_elpd_loo", worst)
    return worst
