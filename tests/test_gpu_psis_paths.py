"""Paths of the Pareto-k kernel the fits of tests/test_gpu_psis.py do not reach, through the testing build
(csrc/ppcx_testing.h): a cutoff value that repeats inside and outside the tail (both parts of the radix selection's tie
branch), a fit's columns over many scratch batches, and the log_p evaluation at other slot counts per launch."""
import numpy as np
import pytest

from tests import psis_restate as R
from tests.gpu_fixtures import testing_library

pytestmark = pytest.mark.gpu


def compare_khat(got, ref, what):
    if np.isinf(ref):
        assert got == ref, (what, got, ref)
    else:
        assert abs(got - ref) <= 1e-12 * abs(ref), (what, got, ref)


@pytest.fixture
def testing_lib():
    with testing_library() as _lib:
        try:
            yield _lib
        finally:
            for key in ("psis_slots", "psis_scratch_bytes"):
                _lib.testing_set(key, 0)


@pytest.mark.parametrize("n", [1000, 5000])
def test_kernel_selection_with_a_repeated_cutoff(testing_lib, n):
    """Poisson values: the (M + 1)-th largest value repeats inside the tail and outside it, so the radix selection takes both
    the keys above its threshold and several copies of the threshold (n = 5000: on the long-column path)"""
    rng = np.random.default_rng(31)
    v = rng.poisson(3.0, size=n).astype(float)
    s = np.sort(v)
    M = R.tail_len(n)
    cut = s[n - M - 1]
    assert (s > cut).sum() > 0 and (s[n - M:] == cut).sum() > 1 and s[n - M] < s[-1]
    cols = np.stack([rng.poisson(2.0, size=n).astype(float), v], axis=1)
    got = testing_lib.testing_psis(v, cols)
    compare_khat(got[-1], R.khat(v), ("ratios", n))
    for i in range(2):
        compare_khat(got[i], R.khat(R.column_values(cols[:, i], v)), ("column", n, i))
    assert np.all(np.isfinite(got))


def test_psis_over_many_scratch_batches_and_slot_counts(testing_lib):
    """The column scratch bounded to 7 columns (every batch boundary of a fit's D columns) and to less than one column give the
    bits of one batch; log_p evaluated 5 or 1 draws per launch instead of 32 (a partial last launch) agrees to 1e-11 and log_g
    to the bit"""
    from ppcseq_amd.synth import synth
    L = testing_lib
    d = synth(40, 12, K=4, seed=3)
    m = L.Model(d["counts"], d["X"], d["exposure"], 4, device=0)
    try:
        f = m.fit_advi(output_samples=1000, iter=2000, seed=6)
        try:
            one = f.psis()
            L.testing_set("psis_scratch_bytes", 8 * 1000 * 7)
            assert np.array_equal(f.psis()["khat"], one["khat"])
            L.testing_set("psis_scratch_bytes", 8)
            assert np.array_equal(f.psis(np.r_[-1, 5, 2], overall=False)["khat"], one["khat"][[-1, 5, 2]])
            L.testing_set("psis_scratch_bytes", 0)
            lp, lg = f.log_ratios()
            dr = f.draws()[0]
            r = R.log_ratios(lp, lg)
            for c in (0, 17, m.D - 1):
                compare_khat(one["khat"][c], R.khat(R.column_values(dr[:, c], r)), c)
        finally:
            f.close()
        for slots in (5, 1):
            L.testing_set("psis_slots", slots)
            g = m.fit_advi(output_samples=1000, iter=2000, seed=6)
            try:
                assert np.array_equal(g.draws()[0], dr)
                lp2, lg2 = g.log_ratios()
                assert np.array_equal(lg2, lg), slots
                assert np.all(np.abs(lp2 - lp) <= 1e-11 * np.maximum(1.0, np.abs(lp))), slots
            finally:
                g.close()
    finally:
        m.close()
