"""The covariance kernel keeps its bits: every key of Fit.loo_moment_match(cov=True), split and unsplit, equal bit for bit, NaN
places included, to what the commit before the local density was stated once for the diagonal and the affine state
(ppcx_loo_mm.h's density over a point accessor, which the kernel now reads under LooMmAffine) returned on an MI355X. The recording is
tests/golden/mm_cov_bits_parent.npz, written by scripts/gpu_record_cell_bits.py --module tests.test_gpu_mm_cov_bits from the
groups below; it holds outputs only, the inputs are the case modules'. tests/test_gpu_mm_bits.py holds the diagonal kernel and
the kernels that run after it in the same way.

designed: each case of loo_mm_cov_cases.designed() on its draw set, with the case's gene, k_threshold, max_iters and r_eff.
widest: the cases of designed(widest=True) (C = 8, 15 and 16). long-n: the prefix of n draws of wide_design_cases' long set
(C = 4), all genes, k_threshold 0.3 -- 6 draws (n <= d + 1), 257 (past the workgroup's stride), 4096 = kPsisLdsDraws (a cell's
arrays in LDS) and 4097 (in the scratch); long-batches runs the 4097 draws in the testing build with the scratch bounded to
batches of two cells and is compared to long-4097's recording.

The recording itself is held to be one of cells that ran: covariance steps on the designed cells and on the outlier cell of
every long group that can have one, and finite values."""
import os

import numpy as np
import pytest

from tests.test_gpu_cell_bits import _items, pack  # noqa: F401  (pack: the recording script's)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mm_cov_bits_parent.npz")
LENGTHS = (6, 257, 4096, 4097)
THRESHOLD = 0.3
GROUPS = ["designed", "widest"] + ["long-%d" % n for n in LENGTHS] + ["long-batches"]
RECORDED = {"long-batches": "long-4097"}              # a group held to another group's recording
COV_CELLS = 8                                         # designed cells with cov_iterations > 0 that the recording must hold
LONG = ["long-%d" % n for n in LENGTHS if n >= 257] + ["long-batches"]   # cov_iterations[0, 5] >= 1, most values finite


def _both(tag, fit, genes, **kw):
    """the two records of the same fit: split and unsplit"""
    return (_items(tag + "/split", fit.loo_moment_match(genes, cov=True, split=True, **kw)) +
            _items(tag + "/unsplit", fit.loo_moment_match(genes, cov=True, **kw)))


def designed(widest=False):
    """the two records of every designed case on its draw set, one model and fit per set"""
    from tests import loo_mm_cov_cases as cov_cases
    from tests.test_gpu_loo_mm import _Held
    held, out = {}, []
    try:
        for c in cov_cases.designed(widest=widest):
            if c["set"] not in held:
                held[c["set"]] = _Held(cov_cases.draw_set(c["set"]))
            S_ = cov_cases.draw_set(c["set"])["counts"].shape[1]
            out += _both(c["name"], held[c["set"]].fit, [c["g"]], r_eff=np.full((1, S_), c["r_eff"]), k_threshold=c["k_threshold"],
                         max_iters=c["max_iters"])
    finally:
        for h in held.values():
            h.close()
    return out


def long_group(lib, n, scratch_bytes=0):
    """the two records of every gene of the long set's first n draws, under the scratch bound where one is given (testing build)"""
    from tests import loo_mm_cases as cases
    from tests import wide_design_cases as W
    from tests.test_gpu_loo_mm import _Held
    h = _Held(cases.prefix(W.draw_set("long"), n))
    try:
        if scratch_bytes:
            lib.testing_set("loo_scratch_bytes", scratch_bytes)
        try:
            return _both("long", h.fit, None, k_threshold=THRESHOLD)
        finally:
            if scratch_bytes:
                lib.testing_set("loo_scratch_bytes", 0)
    finally:
        h.close()


def evaluate(lib, group, testing_path):
    """the (name, array) pairs of a group: the bounded scratch from the testing build at testing_path, the rest from the library
    that is bound now"""
    if group in ("designed", "widest"):
        return designed(widest=group == "widest")
    if group != "long-batches":
        return long_group(lib, int(group.partition("-")[2]))
    lib.use_library(testing_path)
    try:
        n = 4097
        return long_group(lib, n, 2 * 8 * 3 * n + 8)
    finally:
        lib.use_library(None)


@pytest.fixture(scope="module")
def lib():
    from ppcseq_amd import _lib
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the product has no CPU fallback")
    return _lib


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("group", GROUPS)
def test_mm_cov_bits(lib, golden, group):
    from ppcseq_amd import build
    items = evaluate(lib, group, build.build_testing())
    ref, r, with_cov = golden[RECORDED.get(group, group)], 0, 0
    assert sum(v.size for _, v in items) == ref.size, (group, sum(v.size for _, v in items), ref.size)
    for name, v in items:
        want = ref[r:r + v.size].reshape(v.shape)
        r += v.size
        assert np.array_equal(v, want, equal_nan=True), (group, name, v, want)
        if name.endswith("/unsplit.cov_iterations"):
            with_cov += int((want > 0).sum())
            if group in LONG:
                assert want[0, 5] >= 1, (group, want[0, 5])               # the outlier cell of the checked gene 0
    # the recording is of cells that took covariance steps, not of early exits
    if group == "designed":
        assert with_cov >= COV_CELLS, (group, with_cov)
    if group in LONG:
        assert np.isfinite(ref).sum() > ref.size // 2, group
