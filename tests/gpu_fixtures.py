"""What the device tests share: the bracket that puts the testing build (csrc/ppcx_testing.h: forced paths, test hooks) in the
product library's place, and the small NUTS fit that several per-cell diagnostics are tested on. Test modules import the
fixtures by name."""
import contextlib

import numpy as np
import pytest


@contextlib.contextmanager
def testing_library():
    """_lib bound to the testing build inside the block, to the product library again after it. The block closes every Model
    and Fit it makes, and uses none that was made outside it."""
    from ppcseq_amd import _lib, build
    _lib.use_library(build.build_testing())
    try:
        yield _lib
    finally:
        _lib.use_library(None)


testing_library.__test__ = False                 # a helper that test modules import by name, not a test


@pytest.fixture
def testing_lib():
    """The testing build for one test that holds no Model or Fit of the product library"""
    with testing_library() as lib:
        yield lib


@pytest.fixture(scope="module")
def small_fit():
    """(model, NUTS fit, synth data) of 30 genes x 10 samples with the cells 3 and 17 excluded, on the product library"""
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(30, 10, K=4, seed=5)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 4, excl=np.array([3, 10 + 7], np.int32), device=0)
    f = m.fit_nuts(chains=4, iter=400, warmup=150, seed=3)
    yield m, f, d
    f.close()
    m.close()
