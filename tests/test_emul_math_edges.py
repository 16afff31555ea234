"""The host twin of tests/test_gpu_math_edges.py: the same grids and bounds (tests/math_edges.py) on the #else branches of
ppcseq_amd/csrc/ppcx_math.h and the cells of ppcx_model.h, through the CPU emulation harness (tests/emul)."""
import ctypes as C

import numpy as np
import pytest

from tests import math_edges as me
from tests.emul_util import P
from tests.test_disp_table import _exact, _rows

FNS = ("fast_rcp", "fast_log", "fast_exp", "table_log", "window_log", "stirling_tails", "stirling_excess", "log_erfc_ratio",
       "cell", "cell_win", "cell_y", "cell_win_y", "sincos_2pi", "lgamma_int1", "rng_exp", "rng_div")   # ppcx_testing.h PPCX_MATH_* (ppcseq_amd._lib.TESTING_MATH)


@pytest.fixture(scope="module")
def ev(emul):
    def run(fn, a, b=None, y=None):
        a = np.ascontiguousarray(a, np.float64).ravel()
        n = a.size
        b = np.ascontiguousarray(np.zeros(n) if b is None else np.broadcast_to(b, (n,)), np.float64)
        y = np.ascontiguousarray(np.zeros(n) if y is None else np.broadcast_to(y, (n,)), np.int32)
        o0, o1 = np.zeros(n), np.zeros(n)
        assert emul.emul_eval_math(FNS.index(fn), n, P(a, C.c_double), P(b, C.c_double), P(y, C.c_int32), P(o0, C.c_double),
                                   P(o1, C.c_double)) == 0
        return o0, o1
    run.host_branch = True                       # tests/math_edges.py: the libm #else branches
    return run


def test_function_ids_match_the_binding():
    from ppcseq_amd import _lib
    assert _lib.TESTING_MATH == FNS


@pytest.mark.parametrize("name", sorted(me.CHECKS))
def test_host_math_edges_match_mpmath(ev, name):
    me.CHECKS[name](ev)


@pytest.mark.parametrize("name", ["low", "mid", "high", "zeros", "mixed", "excluded"])
def test_host_dispersion_table_at_panel_edges(emul, name):
    """the host build of the tables (ppcx_disp.h) at every panel boundary, the doubles beside it and 1e-3 to either side, at
    test_disp_table's bound"""
    row = _rows()[name]
    sig = []
    for j in range(33):
        b = -8.0 + 0.5 * j
        sig += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf), b - 1e-3, b + 1e-3]
    sig = np.array([s for s in sig if -8.0 <= s < 8.0])
    n = sig.size
    F = np.zeros(n); D = np.zeros(n); Fd = np.zeros(n); Dd = np.zeros(n); inr = np.zeros(n, np.int32)
    emul.emul_disp_table(P(row, C.c_int32), int(row.size), n, P(sig, C.c_double), P(F, C.c_double), P(D, C.c_double),
                         P(Fd, C.c_double), P(Dd, C.c_double), P(inr, C.c_int))
    assert inr[sig != np.nextafter(8.0, 0.0)].all()      # 8 - ulp: (sigma + 8) * 2 rounds to 32, the first direct evaluation
    for i in range(n):
        eF, eD = _exact(row, float(sig[i]))
        for got, ex in ((F[i], eF), (D[i], eD)):
            assert abs(got - float(ex)) <= 8e-16 * float(abs(ex)) + 1e-13, (name, sig[i], got, float(ex))
