"""The per-cell kernels keep their bits: every field of loo, loo_mcse, loo_approx, loo_predict, loo_predict_approx, ppc_exact,
loo_predict_exact (and its ADVI form), loo_moment_match and relative_eff equal bit for bit to what the commit before their
weights stage, exact sweeps and launch path were stated once (ppcx_loo_dev.h loo_cell_weights, cells_in_batches; ppcx_ppc_exact.h
ppc_exact_sweeps) returned on an MI355X. The recording is tests/golden/cell_bits_parent.npz, written by
scripts/gpu_record_cell_bits.py from the groups below; it holds outputs only, the inputs are the case modules'.

Both input forms: host-given columns through the testing hooks (the designed columns of loo_exact_cases, loo_predict_cases,
loo_ap_cases and loo_mcse_cases: ties, cutoff copies, NaN and Inf exits, excluded cells; and long_columns at every LENGTH) and
fits: Model.fit_from_draws over draws of a synthetic model of 6 genes (3 checked) x 5 samples with two excluded cells and one
planted outlier, r_eff absent and given, at every LENGTH, and an ADVI fit of the same model for the three ADVI entries.
LENGTHS: one draw; 20 (the tail would be 4 < 5 draws: no fit); 300; 4096 = kPsisLdsDraws (a cell's arrays in LDS) and 4097 (in
the scratch). One group runs the 4097-draw fit in the testing build with the scratch bounded to two genes' table: three gene
batches, and two (loo, relative_eff) to five (the three-array kernels) cell batches in each."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_bits_parent.npz")
LENGTHS = (1, 20, 300, 4096, 4097)
CHAINS = {1: 1, 20: 2, 300: 3, 4096: 4, 4097: 1}     # of the fit (and of relative_eff on the columns) at each length
G, S, K = 6, 5, 3
EXCL = (0 * S + 2, 4 * S + 0)                         # a cell of a checked gene and one of a plain gene
ADVI_SAMPLES = (300, 4097)
GROUPS = (["designed-exact", "designed-predict", "designed-ap", "designed-mcse"] + ["columns-%d" % n for n in LENGTHS] +
          ["fit-%d" % n for n in LENGTHS] + ["fit-batches"] + ["advi-%d" % n for n in ADVI_SAMPLES])


def _items(prefix, res):
    """a result dict's arrays (or one array) as (name, float64 array) pairs in a fixed order"""
    if isinstance(res, np.ndarray):
        return [(prefix, res.astype(np.float64))]
    return [(prefix + "." + k, np.asarray(v).astype(np.float64)) for k, v in sorted(res.items())
            if isinstance(v, np.ndarray) and k != "genes"]


def designed_exact(lib):
    from tests import loo_exact_cases
    out = []
    for c in loo_exact_cases.designed():
        if c["refused"]:
            continue
        col = lambda k: c[k][:, None]                                     # noqa: E731
        ex, re, nm = [int(c["excluded"])], [c["r_eff"]], c["name"]
        kw = dict(truncation_compensation=c["tc"], p_lo=c["p_lo"], p_hi=c["p_hi"], raw=True)
        form = dict(r_eff=re) if c["lr"] is None else dict(log_ratio=c["lr"])
        out += _items(nm + "/loo_exact", lib.testing_loo_exact(col("ll"), col("eta"), col("sg"), [c["y"]], excluded=ex, **form, **kw))
        out += _items(nm + "/ppc_exact", lib.testing_ppc_exact(col("eta"), col("sg"), [c["y"]], ex, **kw))
        if c["lr"] is None:
            out += _items(nm + "/loo", lib.testing_loo(col("ll"), ex, re))
            out += _items(nm + "/loo_mcse", lib.testing_loo_mcse(col("ll"), ex, re))
    return out


def designed_predict(lib):
    from tests import loo_predict_cases
    out = []
    for c in loo_predict_cases.designed():
        out += _items(c["name"], lib.testing_loo_predict(c["ll"][:, None], c["x"][:, None], [c["y"]], [int(c["excluded"])], [c["r_eff"]],
                                                         c["p_lo"], c["p_hi"]))
    return out


def designed_ap(lib):
    from tests import loo_ap_cases
    out = []
    for name, ll, a, excl in loo_ap_cases.designed():
        out += _items(name + "/loo_approx", lib.testing_loo_approx(ll[:, None], a, [int(excl)]))
    for name, ll, a, x, y, excl, p_lo, p_hi in loo_ap_cases.predictive():
        out += _items(name + "/loo_predict_approx", lib.testing_loo_predict_approx(ll[:, None], a, x[:, None], [y], [int(excl)], p_lo, p_hi))
    return out


def designed_mcse(lib):
    from tests import loo_mcse_cases
    out = []
    for which, (ll, excl, r_eff) in (("designed", loo_mcse_cases.designed()), ("small", loo_mcse_cases.small())):
        for re in (None, r_eff):
            tag = "%s/r_eff %s" % (which, "absent" if re is None else "given")
            out += _items(tag + "/loo", lib.testing_loo(ll, excl, re))
            out += _items(tag + "/loo_mcse", lib.testing_loo_mcse(ll, excl, re))
    return out


def columns(lib, n):
    """every hook on the long columns of n draws"""
    from tests import loo_ap_cases, loo_exact_cases, loo_predict_cases
    from tests.ppc_exact_restate import P2, TC
    out = []
    ll, eta, sg, y, excl, r_eff, lr = loo_exact_cases.long_columns(n)
    kw = dict(truncation_compensation=TC, p_lo=P2, p_hi=1 - P2, raw=True)
    out += _items("loo_exact", lib.testing_loo_exact(ll, eta, sg, y, excluded=excl, r_eff=r_eff, **kw))
    out += _items("loo_exact_approx", lib.testing_loo_exact(ll, eta, sg, y, excluded=excl, log_ratio=lr, **kw))
    out += _items("ppc_exact", lib.testing_ppc_exact(eta, sg, y, excl, **kw))
    for tag, re in (("absent", None), ("given", r_eff)):
        out += _items("loo/r_eff " + tag, lib.testing_loo(ll, excl, re))
        out += _items("loo_mcse/r_eff " + tag, lib.testing_loo_mcse(ll, excl, re))
    out += _items("loo_approx", lib.testing_loo_approx(ll, lr, excl))
    out += _items("relative_eff", lib.testing_relative_eff(ll, CHAINS[n]))
    ll, x, y = loo_predict_cases.long_columns(n)
    excl = np.zeros(ll.shape[1], np.int32)
    excl[-1] = 1
    out += _items("loo_predict", lib.testing_loo_predict(ll, x, y, excl, np.linspace(0.4, 1.0, ll.shape[1])))
    out += _items("loo_predict/r_eff absent", lib.testing_loo_predict(ll, x, y))
    ll, a, x, y, excl = loo_ap_cases.long_columns(n)
    out += _items("loo_predict_approx", lib.testing_loo_predict_approx(ll, a, x, y, excl))
    return out


def model_inputs():
    """counts [G, S], X [S, 2], exposure [S] of the synthetic model; cell (1, 3) carries a planted outlier"""
    from ppcseq_amd.synth import synth
    d = synth(G, S, K=K, seed=20261)
    counts = np.array(d["counts"], np.int32).copy()
    counts[1, 3] = 40 * counts[1, 3] + 400
    return counts, np.asarray(d["X"], np.float64), np.asarray(d["exposure"], np.float64)


def fit_draws(n):
    """[CHAINS[n], n / CHAINS[n], D] unconstrained draws around the data's own parameters, the hyper-parameters of loo_mm_cases"""
    from tests import loo_mm_cases
    counts, X, expo = model_inputs()
    d = loo_mm_cases.dims(G, 2, K)
    rng = np.random.default_rng(300 + n)
    u = rng.normal(0.0, 0.05, (n, d["D"]))
    h = loo_mm_cases.HYPER[None, :] + rng.normal(0.0, 0.02, (n, 6))
    u[:, 0:3], u[:, d["tail"]:d["tail"] + 3] = h[:, :3], h[:, 3:]
    u[:, d["intercept"]:d["intercept"] + G] = np.log(counts.mean(axis=1) + 1.0)[None, :] + rng.normal(0.0, 0.25, (n, G))
    u[:, d["alpha1"]:d["alpha1"] + K] = rng.normal(0.0, 0.3, (n, K))
    u[:, d["sigma_raw"]:d["sigma_raw"] + G] = rng.normal(-1.0, 0.3, (n, G))
    return np.ascontiguousarray(u.reshape(CHAINS[n], n // CHAINS[n], d["D"]))


def _model(lib):
    from tests import loo_mm_cases
    counts, X, expo = model_inputs()
    return lib.Model(counts, X, expo, K, lambda_mu_mu=loo_mm_cases.LAMBDA_MU_MU, excl=np.array(EXCL, np.int32), device=0)


def fit_entries(fit):
    """every NUTS entry of a fit, r_eff absent and given"""
    from tests.ppc_exact_restate import P2, TC
    given = np.linspace(0.4, 1.0, G * S).reshape(G, S)
    kw = dict(p_lo=P2, p_hi=1 - P2, truncation_compensation=TC)
    out = _items("relative_eff", fit.relative_eff())
    out += _items("ppc_exact", fit.ppc_exact(**kw))
    for tag, re in (("absent", None), ("given", given)):
        out += _items("loo/r_eff " + tag, fit.loo(r_eff=re))
        if fit.chains * fit.n_keep > 1:                                   # (Fit.loo's mcse total is not defined at one draw)
            out += _items("loo_mcse/r_eff " + tag, fit.loo(r_eff=re, mcse=True))
        out += _items("loo_predict/r_eff " + tag, fit.loo_predict(r_eff=re, seed=3, **kw))
        out += _items("loo_predict_exact/r_eff " + tag, fit.loo_predict_exact(r_eff=None if re is None else re[:K], **kw))
        out += _items("loo_moment_match/r_eff " + tag, fit.loo_moment_match(r_eff=re, k_threshold=0.5, max_iters=4))
    return out


def fit_group(lib, n, scratch_bytes=0):
    m = _model(lib)
    try:
        f = m.fit_from_draws(fit_draws(n))
        try:
            if scratch_bytes:
                lib.testing_set("loo_scratch_bytes", scratch_bytes)
            try:
                return fit_entries(f)
            finally:
                if scratch_bytes:
                    lib.testing_set("loo_scratch_bytes", 0)
        finally:
            f.close()
    finally:
        m.close()


def advi_group(lib, n):
    from tests.ppc_exact_restate import P2, TC
    kw = dict(p_lo=P2, p_hi=1 - P2, truncation_compensation=TC)
    m = _model(lib)
    try:
        f = m.fit_advi(output_samples=n, iter=400, eval_elbo=50, seed=4)
        try:
            out = _items("loo_approx", f.loo_approximate_posterior())
            out += _items("loo_predict_approx", f.loo_predict_approximate_posterior(seed=3, **kw))
            out += _items("loo_predict_exact_approx", f.loo_predict_exact_approximate_posterior(**kw))
            return out
        finally:
            f.close()
    finally:
        m.close()


def evaluate(lib, group, testing_path):
    """the (name, array) pairs of a group: the hooks and the bounded scratch from the testing build at testing_path, the fits
    from the library that is bound now"""
    kind, _, arg = group.partition("-")
    if kind == "fit" and arg != "batches":
        return fit_group(lib, int(arg))
    if kind == "advi":
        return advi_group(lib, int(arg))
    lib.use_library(testing_path)
    try:
        if kind == "fit":
            n = 4097
            return fit_group(lib, n, 2 * 8 * 3 * n + 8)
        if kind == "columns":
            return columns(lib, int(arg))
        return {"exact": designed_exact, "predict": designed_predict, "ap": designed_ap, "mcse": designed_mcse}[arg](lib)
    finally:
        lib.use_library(None)


def pack(items):
    """a group's arrays end to end (one archive member per array would cost the file more in headers than in data)"""
    return np.concatenate([v.ravel() for _, v in items])


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
def test_cell_bits(lib, golden, group):
    from ppcseq_amd import build
    items = evaluate(lib, group, build.build_testing())
    ref, r = golden[group], 0
    assert sum(v.size for _, v in items) == ref.size, (group, sum(v.size for _, v in items), ref.size)
    for name, v in items:
        want = ref[r:r + v.size].reshape(v.shape)
        r += v.size
        assert np.array_equal(v, want, equal_nan=True), (group, name, v, want)
    if group.split("-")[0] in ("fit", "columns", "advi") and group.split("-")[1] not in ("1", "20"):
        assert np.isfinite(ref).sum() > ref.size // 2, group             # the recording is of cells that ran, not of NaN exits
