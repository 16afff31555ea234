"""The scalar building blocks of the log density and of the predictive sampler (ppcseq_amd/csrc/ppcx_math.h, the cells of ppcx_model.h) at their edges --
binade and bin boundaries, the ends of the tables, rint ties, underflow -- against mpmath at 40 digits. Shared by the device
run (tests/test_gpu_math_edges.py: the testing build's ppcx_testing_eval_math, the gfx950 branches and the LDS tables) and its
host twin (tests/test_emul_math_edges.py: the #else branches through tests/emul).

Each check_* takes ev(fn, a, b=None, y=None) -> (out0, out1) with the function names of ppcseq_amd._lib.TESTING_MATH."""
import math

import mpmath as mp
import numpy as np

DPS = 40
TINY = 2.0 ** -1074                              # the subnormal spacing


def _nb(x, k=1):
    """x and its k nearest neighbours on both sides."""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, float)))


def _ref(f, xs):
    with mp.workdps(DPS):
        return [f(mp.mpf(float(x))) for x in xs]


def _abs_err(got, ref):
    with mp.workdps(DPS):
        return np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(got, ref)])


def _report(name, x, err, tol):
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, f"{name}: {bad.size} of {len(x)} points off, worst at x = {np.asarray(x)[bad[np.argmax((err / tol)[bad])]]!r} " \
                          f"(error {np.max(err[bad]):.3g}, bound {tol[bad][np.argmax((err / tol)[bad])]:.3g})"


# ---- fast_rcp --------------------------------------------------------------------------------------------------------
def rcp_grid():
    rng = np.random.default_rng(1)
    g = list(np.linspace(1.0, 2.0, 4001)[:-1]) + list(rng.uniform(1.0, 2.0, 4000))
    for k in range(-3, 1021):
        g += _nb(2.0 ** k)
    g += list(2.0 + np.linspace(math.sqrt(0.5) - 1.0, math.sqrt(2.0) - 1.0, 2001))     # what fast_log divides by
    return np.array([v for v in g if v > 0])


def check_fast_rcp(ev):
    x = rcp_grid()
    got, _ = ev("fast_rcp", x)
    ref = _ref(lambda v: 1 / v, x)
    err = _abs_err(got, ref) / np.abs(1.0 / x)
    _report("fast_rcp", x, err, np.full(x.size, 2.2e-15))


# ---- fast_log --------------------------------------------------------------------------------------------------------
def log_grid():
    g = []
    for k in range(-8, 9):                                         # the lo split m = sqrt(1/2) in several binades
        g += _nb(math.ldexp(math.sqrt(0.5), k), 3)
        g += _nb(math.ldexp(math.sqrt(2.0), k), 3)
    g += _nb(1.0, 64)
    for k in range(-1074, 1024, 7):
        g += _nb(2.0 ** k)
    g += [TINY, 3 * TINY, 2.0 ** -1050 * 1.5, 2.0 ** -1023, 1e-320, 1e-310, 1.7976931348623157e308, 1e308]
    g += list(np.geomspace(1e-320, 1e308, 3000))
    return np.array([v for v in g if 0 < v < np.inf])


def check_fast_log(ev):
    x = log_grid()
    got, _ = ev("fast_log", x)
    ref = _ref(mp.log, x)
    err = _abs_err(got, ref)
    # 2 units in the last place of ln x; near x = 1, where ln x -> 0, the error of ln(1 + f) with f exact (fdlibm: < 1 ulp)
    tol = np.maximum(2 * _ulp([float(r) for r in ref]), np.where(np.abs(x - 1.0) < 0.5, 0.0, 2.3e-16))
    tol = np.where(x == 1.0, 0.0, tol)
    _report("fast_log", x, err, tol)


# ---- fast_exp --------------------------------------------------------------------------------------------------------
def exp_grid():
    ln2 = math.log(2.0)
    g = []
    for k in range(-1076, 1024, 3):                                 # the rint ties of x / ln 2
        g += _nb((k + 0.5) * ln2)
    g += [0.0, -0.0, 1e-300, -1e-300, TINY, -TINY, 1e-17, -1e-17, 709.78, 709.782712893384]
    g += list(np.linspace(-745.0, -708.0, 3001))                    # subnormal results
    g += list(np.linspace(-700.0, 700.0, 2001))
    return np.array([v for v in g if -745.13 < v < 709.7827])


def check_fast_exp(ev):
    x = exp_grid()
    got, _ = ev("fast_exp", x)
    ref = _ref(mp.exp, x)
    err = _abs_err(got, ref)
    rf = np.array([float(r) for r in ref])
    tol = 2 * _ulp(rf) + np.where(rf < 2.0 ** -1022, TINY, 0.0)  # below the normal range: one subnormal spacing more
    _report("fast_exp", x, err, tol)


# ---- table_log, window_log -------------------------------------------------------------------------------------------
def _bin_points(lo, bits):
    """start, start + ulp, centre, next start - ulp of every bin of the top `bits` mantissa bits in the binade [lo, 2 lo)"""
    n = 1 << bits
    out = []
    for j in range(n):
        s = lo * (1.0 + j / n)
        e = lo * (1.0 + (j + 1) / n)
        out += [s, np.nextafter(s, np.inf), lo * (1.0 + (j + 0.5) / n), np.nextafter(e, -np.inf)]
    return out


def table_log_grid():
    g = []
    for e in (0, 1, 3, 7, 52, 200, 996):
        g += _bin_points(2.0 ** e, 8)
    g += list(np.geomspace(1.0, 1e300, 2000))
    return np.array(g)


def _log_tol(ref):
    return 4.5e-16 * np.maximum(1.0, np.abs(np.array([float(r) for r in ref])))


def check_table_log(ev):
    x = table_log_grid()
    got, _ = ev("table_log", x)
    ref = _ref(mp.log, x)
    _report("table_log", x, _abs_err(got, ref), _log_tol(ref))


def window_grid():
    g = []
    for e in range(4):
        g += _bin_points(2.0 ** e, 8)
    g.append(np.nextafter(16.0, 0.0))
    return np.array(g)


def check_window_log(ev):
    x = window_grid()
    got, _ = ev("window_log", x)
    ref = _ref(mp.log, x)
    _report("window_log", x, _abs_err(got, ref), _log_tol(ref))


# ---- the cells -------------------------------------------------------------------------------------------------------
YS = (0, 1, 7, 8, 2 ** 31 - 1)


def _cell_w(e, A):
    """w = fma(e, A, 1) as the cell forms it (one rounding)"""
    with mp.workdps(700):
        return np.array([float(mp.mpf(float(a)) * mp.mpf(float(b)) + 1) for a, b in zip(e, A)])


def _check_cell(ev, fn, e, A, name):
    w = _cell_w(e, A)
    for y in YS:
        l, q = ev(fn, e, A, y)
        refl = _ref(mp.log, w)
        _report(f"{name} ln w (y = {y})", w, _abs_err(l, refl), _log_tol(refl))
        _report(f"{name} q (y = {y})", w, _abs_err(q, _ref(lambda v: 1 / v, w)) / (1.0 / w), np.full(w.size, 2.2e-15))
        sa, syq = ev(fn + "_y", e, A, y)
        # the count is converted exactly: y ln w and y q are the single roundings of the products
        assert np.array_equal(sa, float(y) * l), (name, y)
        assert np.array_equal(syq, float(y) * q), (name, y)


def check_cell(ev):
    w = table_log_grid()
    w = w[w >= 2.0]                                  # e = w - 1 is exact up to 2^53; beyond, fma(w, 1, 1) = w
    e = np.where(w < 2.0 ** 53, w - 1.0, w)
    _check_cell(ev, "cell", e, np.ones_like(e), "cell_eval")
    # the same w from an exposure and a gene constant that are not 1: w = fma(e, A, 1) rounded once
    rng = np.random.default_rng(3)
    A = np.exp(rng.uniform(-3, 3, w.size))
    _check_cell(ev, "cell", e / A, A, "cell_eval (e A)")


def check_cell_win(ev):
    w = window_grid()
    w = w[w > 1.0]
    _check_cell(ev, "cell_win", w - 1.0, np.ones_like(w), "cell_eval_win")       # w - 1 exact below 16


# ---- Stirling ----------------------------------------------------------------------------------------------------------
def _lg_tail(x):
    return mp.loggamma(x) - ((x - mp.mpf(0.5)) * mp.log(x) - x + mp.log(2 * mp.pi) / 2)


def _dg_tail(x):
    return mp.log(x) - mp.digamma(x)


def check_stirling_tails(ev):
    xs = list(np.geomspace(8.0, 1e6, 600)) + _nb(8.0)[0:1] + _nb(32.0) + _nb(256.0) + [np.nextafter(8.0, np.inf), 1e6]
    r = 1.0 / np.array(xs)
    lg, dg = ev("stirling_tails", r)
    with mp.workdps(DPS):
        xr = [1 / mp.mpf(float(v)) for v in r]                   # the argument the tails see: 1/r exactly
        ref_lg = [_lg_tail(v) for v in xr]
        ref_dg = [_dg_tail(v) for v in xr]
    _report("stirling_tails lg", r, _abs_err(lg, ref_lg), np.full(r.size, 6e-16))
    _report("stirling_tails dg", r, _abs_err(dg, ref_dg), np.full(r.size, 6e-16))


def check_stirling_excess(ev):
    phi = np.concatenate([np.geomspace(1.7e-4, 1e4, 800), _nb(8.0, 2), [1.0, 2.0, 7.0, 7.5]])
    with mp.workdps(DPS):
        lnphi = np.array([float(mp.log(mp.mpf(float(p)))) for p in phi])
        ref_d = [_lg_tail(mp.mpf(float(p))) for p in phi]
        ref_p = [_dg_tail(mp.mpf(float(p))) for p in phi]
    dl1, dp1 = ev("stirling_excess", phi, lnphi, 1)
    for got, ref, nm in ((dl1, ref_d, "dlt"), (dp1, ref_p, "dps")):
        tol = 1e-14 * np.maximum(1.0, np.abs(np.array([float(v) for v in ref])))
        _report(f"stirling_excess {nm}", phi, _abs_err(got, ref), tol)
    big = phi >= 8.0                                 # any_small only selects the form of the lanes below 8
    dl0, dp0 = ev("stirling_excess", phi[big], lnphi[big], 0)
    assert np.array_equal(dl0, dl1[big]) and np.array_equal(dp0, dp1[big])


# ---- log erfc and the ratio of the skew-normal prior --------------------------------------------------------------------
def last_erfc_positive():
    """the largest double x with erfc(x) >= half the smallest subnormal (so that it rounds to > 0)"""
    lo, hi = 26.0, 27.5
    with mp.workdps(DPS):
        half = mp.mpf(2) ** -1075
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid in (lo, hi):
                break
            if mp.erfc(mid) > half:
                lo = mid
            else:
                hi = mid
    return lo


def erfc_grid():
    xl = last_erfc_positive()
    g = list(np.linspace(-30.0, 27.5, 2301)) + list(np.linspace(26.3, 26.7, 801)) + _nb(xl, 2) + _nb(math.sqrt(700.0), 2)
    g += [0.0, -0.0, 1e-300, 26.40, 26.46, 26.50, 26.55, 26.60, 26.64, 26.65, 27.0, 27.3]
    return np.array(g)


def check_log_erfc_ratio(ev):
    x = erfc_grid()
    le, ra = ev("log_erfc_ratio", x)
    with mp.workdps(DPS):
        for i, v in enumerate(x):
            e = mp.erfc(mp.mpf(float(v)))
            if not np.isfinite(le[i]):
                # erfc(x) = 0 in double precision: only where it is below two subnormal spacings (at the last two, either
                # rounding of erfc is allowed)
                assert e < mp.mpf(2) ** -1073 and le[i] == -np.inf and np.isnan(ra[i]), (v, le[i], ra[i], e)
                continue
            assert e > mp.mpf(2) ** -1076 and np.isfinite(ra[i]), (v, le[i], ra[i], e)
            # a subnormal erfc carries up to 4 of its spacings more (the resolution of Stan's quotient too)
            sub = float(4 * mp.mpf(2) ** -1074 / e) if e < mp.mpf(2) ** -1022 else 0.0
            lref = mp.log(e)
            rref = mp.exp(-mp.mpf(float(v)) ** 2) / e
            # log erfc: relative, with the half unit of 1 that the rounding of erfc near 1 leaves in the log
            tl = 1e-13 * abs(float(lref)) + math.log1p(sub) + 2.3e-16
            assert abs(le[i] - float(lref)) <= tl, ("log_erfc", v, le[i], float(lref))
            # the ratio: relative; where it is itself below the normal range, two of its spacings
            tr = (1e-13 + sub) * float(rref) + 2 * TINY
            assert abs(ra[i] - float(rref)) <= tr, ("ratio", v, ra[i], float(rref), float(e))

# ---- the predictive sampler's own functions (ppcx_math.h: sincos_2pi, lgamma_int1, rng_exp, rng_div) ------------------------------
# On the device these are hand-written (a quadrant reduction on u with the fdlibm kernels, a table and Stirling, fast_exp inside
# a guard, a multiplication by fast_rcp); on the host they are libm. An evaluator of the host branch says so with an attribute
# `host_branch`: where the two branches' bounds differ, each is held to the one that follows from its own code.
WORST = {}                                       # name -> the worst error of the last run, in the unit of its bound


def sincos_grid():
    g = []
    for k in range(1, 8):                        # k/8 (and with it k/4): where flip and the quadrant change
        g += _nb(k / 8.0, 2)
    g += _nb(2.0 ** -54, 2)[0:1] + [np.nextafter(2.0 ** -54, 1.0), 1.0 - 2.0 ** -54, np.nextafter(1.0 - 2.0 ** -54, 0.0)]   # the ends of u01
    g += list(np.random.default_rng(11).uniform(0.0, 1.0, 10000))
    return np.array([v for v in g if 0.0 < v < 1.0])


def check_sincos_2pi(ev):
    u = sincos_grid()
    sn, cs = ev("sincos_2pi", u)
    with mp.workdps(DPS):
        ang = [2 * mp.pi * mp.mpf(float(v)) for v in u]
        rs, rc = [mp.sin(a) for a in ang], [mp.cos(a) for a in ang]
    es, ec = _abs_err(sn, rs), _abs_err(cs, rc)
    # device: r = u - q/4 and the flip are exact, t = r 2pi carries one rounding and the constant's error at t <= pi/4
    # (5.5e-17 + 3.1e-17) and the fdlibm kernels stay below 1 ulp (1.1e-16): below 2^-52 in all; 2^-51 is asserted.
    # host: t = fl(2pi) u up to 2 pi carries the constant's 2.5e-16 and half an ulp of t (4.4e-16) before libm's sine: 2^-50.
    tol = 2.0 ** -50 if getattr(ev, "host_branch", False) else 2.0 ** -51
    WORST["sincos_2pi"] = float(max(es.max(), ec.max()))
    _report("sincos_2pi sin", u, es, np.full(u.size, tol))
    _report("sincos_2pi cos", u, ec, np.full(u.size, tol))
    # the quadrant: signs wherever the exact value is beyond the bound, and at k/4 the unit component exactly
    for got, ref, nm in ((sn, rs, "sin"), (cs, rc, "cos")):
        rf = np.array([float(r) for r in ref])
        big = np.abs(rf) > tol
        assert np.array_equal(np.sign(got[big]), np.sign(rf[big])), f"sincos_2pi {nm}: wrong sign"
    for k, (s_, c_) in ((1, (1.0, 0.0)), (2, (0.0, -1.0)), (3, (-1.0, 0.0))):
        s1, c1 = ev("sincos_2pi", np.array([k / 4.0]))
        if s_ != 0.0:
            assert s1[0] == s_ and abs(c1[0]) <= tol, (k, s1[0], c1[0])
        else:
            assert c1[0] == c_ and abs(s1[0]) <= tol, (k, s1[0], c1[0])
        if not getattr(ev, "host_branch", False):
            assert (c1[0] if s_ != 0.0 else s1[0]) == 0.0, (k, s1[0], c1[0])      # the reduced argument is exactly 0


def lgamma_int_grid():
    g = [8.0, 9.0, 10.0]
    for j in range(4, 32):                       # up to 2^31: the largest kf a PTRS proposal with lambda < 2^30 can reach
        g += [2.0 ** j - 1.0, 2.0 ** j, 2.0 ** j + 1.0]
    g += list(np.floor(np.exp(np.random.default_rng(12).uniform(math.log(8.0), math.log(2.0 ** 31), 2000))))
    return np.array(g)


def check_lgamma_int1(ev):
    k = np.arange(8.0)                           # the table: ln k! to one unit in the last place
    got, _ = ev("lgamma_int1", k)
    ref = _ref(lambda v: mp.loggamma(v + 1), k)
    err = _abs_err(got, ref)
    _report("lgamma_int1 table", k, err, np.maximum(_ulp([float(r) for r in ref]), 0.0) * (k >= 2))
    k = lgamma_int_grid()
    got, _ = ev("lgamma_int1", k)
    ref = _ref(lambda v: mp.loggamma(v + 1), k)
    err = _abs_err(got, ref)
    x = k + 1.0
    unit = _ulp(x * np.log(x))                   # (x - 1/2) ln x, its product with x and the sum: three rounded terms of that size
    WORST["lgamma_int1"] = float(np.max(err / unit))
    _report("lgamma_int1", k, err, 4 * unit)


def rng_exp_grid():
    g = []
    for v in (699.999, 700.0):
        g += _nb(v, 2) + _nb(-v, 2)
    g += [709.7, -709.7, -745.2, 710.0, -746.0, 705.0, -705.0, -720.0, 0.0, 1.0, -1.0]
    return np.array(g)


def check_rng_exp(ev):
    x = rng_exp_grid()
    got, _ = ev("rng_exp", x)
    assert got[x == 710.0][0] == np.inf and got[x == -746.0][0] == 0.0
    fin = (x != 710.0) & (x != -746.0)
    x, got = x[fin], got[fin]
    ref = _ref(mp.exp, x)
    rf = np.array([float(r) for r in ref])
    err = _abs_err(got, ref)
    # inside the guard fast_exp's bound (check_fast_exp), outside libm's one unit in the last place (of the subnormal spacing
    # where the result is subnormal)
    inside = (x > -700.0) & (x < 700.0)
    tol = np.where(inside, 2 * _ulp(rf), np.maximum(_ulp(rf), TINY))
    WORST["rng_exp"] = float(np.max(err / np.maximum(_ulp(rf), TINY)))
    _report("rng_exp", x, err, tol)


def check_rng_div(ev):
    b = rcp_grid()
    rng = np.random.default_rng(13)
    a = np.exp(rng.uniform(-20.0, 20.0, b.size)) * rng.choice([-1.0, 1.0], b.size)
    keep = (np.abs(a / b) > 1e-290) & (np.abs(a / b) < 1e290) & (b < 1e300)          # normal quotients of normal operands
    a, b = a[keep], b[keep]
    got, _ = ev("rng_div", a, b)
    with mp.workdps(DPS):
        ref = [mp.mpf(float(p)) / mp.mpf(float(q)) for p, q in zip(a, b)]
    err = _abs_err(got, ref)
    unit = _ulp([float(r) for r in ref])
    WORST["rng_div"] = float(np.max(err / unit))
    _report("rng_div", b, err, 2 * unit)


CHECKS = {
    "fast_rcp": check_fast_rcp, "fast_log": check_fast_log, "fast_exp": check_fast_exp, "table_log": check_table_log,
    "window_log": check_window_log, "cell": check_cell, "cell_win": check_cell_win, "stirling_tails": check_stirling_tails,
    "stirling_excess": check_stirling_excess, "log_erfc_ratio": check_log_erfc_ratio,
    "sincos_2pi": check_sincos_2pi, "lgamma_int1": check_lgamma_int1, "rng_exp": check_rng_exp, "rng_div": check_rng_div,
}
