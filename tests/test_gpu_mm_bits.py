"""The moment-matched kernels keep their bits: every field of loo_moment_match and loo_predict_exact_moment_match, split and
unsplit (the four records of tests/test_gpu_loo_mm_split.py's _both), equal bit for bit, NaN places included, to what the commit
before their shared stages and driver were stated once (ppcx_loo_dev.h loo_exact_cell, loo_fill_eta_lnphi; ppcx_loo_mm_dev.h
loo_mm_count_ratios, loo_mm_lpd, loo_mm_weighted_elpd, loo_mm_then_fit_cells) returned on an MI355X. The recording is
tests/golden/mm_bits_parent.npz, written by scripts/gpu_record_cell_bits.py --module tests.test_gpu_mm_bits from the groups below;
it holds outputs only, the inputs are the case modules'. tests/test_gpu_cell_bits.py holds loo_predict_exact and
loo_moment_match on its own fits in the same way.

designed: each case of loo_mm_cases.designed() on its draw set with every gene checked, with the case's gene, k_threshold,
max_iters and r_eff. long-n: the prefix of n draws of the long set, genes 0 and 1, k_threshold 0.7 -- one draw, three (h = 1),
257 (past the workgroup's stride), 512 (h on a stride boundary), 4096 = kPsisLdsDraws (a cell's arrays in LDS) and 4097 (in the
scratch); long-batches runs the 4097 draws in the testing build with the scratch bounded to gene batches of two and cell batches
of two and is compared to long-4097's recording. wide-C3, wide-C4: the designed cells of tests/wide_design_cases.py (the
predictive forms for the checked genes, as the entry takes them), wide-C4 also the 4 097 draws of its long set under the bound
tests/test_gpu_wide_designs.py sets (testing build).

The recording itself is held to be one of cells that ran: matched cells in every group that can have them, and finite values."""
import os

import numpy as np
import pytest

from tests.test_gpu_cell_bits import _items, pack  # noqa: F401  (pack: the recording script's)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mm_bits_parent.npz")
LENGTHS = (1, 3, 257, 512, 4096, 4097)
TC = 0.7352941
GROUPS = ["designed"] + ["long-%d" % n for n in LENGTHS] + ["long-batches", "wide-C3", "wide-C4"]
RECORDED = {"long-batches": "long-4097"}              # a group held to another group's recording
# cells with iterations > 0 that the recording must hold (the unsplit elpd record), by group
MATCHED = dict({"designed": 8, "wide-C3": 1, "wide-C4": 1, "long-batches": 1}, **{"long-%d" % n: 1 for n in LENGTHS if n >= 257})


def _four(tag, fit, genes, xgenes, **kw):
    """the four records of the same fit: elpd form split / unsplit (genes), predictive form split / unsplit (xgenes: checked)"""
    xkw = dict(kw, truncation_compensation=TC)
    return (_items(tag + "/split", fit.loo_moment_match(genes, split=True, **kw)) +
            _items(tag + "/unsplit", fit.loo_moment_match(genes, **kw)) +
            _items(tag + "/exact split", fit.loo_predict_exact_moment_match(xgenes, split=True, **xkw)) +
            _items(tag + "/exact unsplit", fit.loo_predict_exact_moment_match(xgenes, **xkw)))


def _held_sets(make, designed):
    """the four records of every designed case on its draw set (make(name)), one model and fit per set; a case of a gene that is
    not checked: the elpd forms alone (the predictive entries take checked genes)"""
    from tests.test_gpu_loo_mm_exact import _Held
    sets, held, out = {}, {}, []
    try:
        for c in designed:
            if c["set"] not in held:
                sets[c["set"]] = make(c["set"])
                held[c["set"]] = _Held(sets[c["set"]])
            ds, fit = sets[c["set"]], held[c["set"]].fit
            re = np.full((1, ds["counts"].shape[1]), c["r_eff"])
            kw = dict(r_eff=re, k_threshold=c["k_threshold"], max_iters=c["max_iters"])
            if c["g"] < ds["K"]:
                out += _four(c["name"], fit, [c["g"]], [c["g"]], **kw)
            else:
                out += _items(c["name"] + "/split", fit.loo_moment_match([c["g"]], split=True, **kw))
                out += _items(c["name"] + "/unsplit", fit.loo_moment_match([c["g"]], **kw))
    finally:
        for h in held.values():
            h.close()
    return out


def designed():
    from tests import loo_mm_cases as cases
    from tests.test_gpu_loo_mm_exact import checked_all
    return _held_sets(lambda name: checked_all(cases.draw_set(name)), cases.designed())


def _prefix_group(lib, ds, tag, scratch_bytes):
    """the four records of every gene of a draw set (the predictive forms: its checked genes) at k_threshold 0.7, under the
    scratch bound where one is given (testing build)"""
    from tests.test_gpu_loo_mm_exact import _Held
    h = _Held(ds)
    try:
        if scratch_bytes:
            lib.testing_set("loo_scratch_bytes", scratch_bytes)
        try:
            return _four(tag, h.fit, np.arange(ds["counts"].shape[0]), np.arange(ds["K"]), k_threshold=0.7)
        finally:
            if scratch_bytes:
                lib.testing_set("loo_scratch_bytes", 0)
    finally:
        h.close()


def long_group(lib, n, scratch_bytes=0):
    from tests import loo_mm_cases as cases
    from tests.test_gpu_loo_mm_exact import checked_all
    return _prefix_group(lib, cases.prefix(checked_all(cases.long_set()), n), "long", scratch_bytes)


def wide_designed(name):
    from tests import wide_design_cases as W
    return _held_sets(W.draw_set, [c for c in W.designed() if c["set"] == name])


def wide_long(lib):
    """tests/test_gpu_wide_designs.py's 4 097 draws under its bound: the gene table in batches of two genes, the cells in
    batches of three"""
    from tests import loo_mm_cases as cases
    from tests import wide_design_cases as W
    n = 4097
    ds = cases.prefix(W.draw_set("long"), n)
    return _prefix_group(lib, ds, "long", 2 * 8 * (ds["X"].shape[1] + 1) * n + 8)


def evaluate(lib, group, testing_path):
    """the (name, array) pairs of a group: the bounded scratch from the testing build at testing_path, the rest from the library
    that is bound now"""
    if group == "designed":
        return designed()
    if group == "wide-C3":
        return wide_designed("covariate")
    if group.startswith("long-") and group != "long-batches":
        return long_group(lib, int(group.partition("-")[2]))
    out = wide_designed("factor4") if group == "wide-C4" else []
    lib.use_library(testing_path)
    try:
        n = 4097
        return out + (wide_long(lib) if group == "wide-C4" else long_group(lib, n, 2 * 8 * 3 * n + 8))
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
def test_mm_bits(lib, golden, group):
    from ppcseq_amd import build
    items = evaluate(lib, group, build.build_testing())
    ref, r, matched = golden[RECORDED.get(group, group)], 0, 0
    assert sum(v.size for _, v in items) == ref.size, (group, sum(v.size for _, v in items), ref.size)
    for name, v in items:
        want = ref[r:r + v.size].reshape(v.shape)
        r += v.size
        assert np.array_equal(v, want, equal_nan=True), (group, name, v, want)
        if name.endswith("/unsplit.iterations"):
            matched += int((want > 0).sum())
    # the recording is of cells that were matched and split, not of early exits
    assert matched >= MATCHED.get(group, 0), (group, matched)
    if group in MATCHED:                                                  # the groups of 257 draws and more
        assert np.isfinite(ref).sum() > ref.size // 2, group
