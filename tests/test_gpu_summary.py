"""ppcx_fit_summary on the MI355X against the numpy restatement (tests/summary_restate.py), its refusals, its determinism, and
the convergence checks of do_inference(check_convergence=True)."""
import warnings

import numpy as np
import pytest

from tests import summary_restate as R

pytestmark = pytest.mark.gpu


def compare(got, i, ref, what):
    for k in ("q05", "q50", "q95"):
        assert got[k][i] == ref[k] or (np.isnan(ref[k]) and np.isnan(got[k][i])), (what, k, got[k][i], ref[k])
    for k, tol, rel in (("mean", 1e-12, True), ("sd", 1e-12, True), ("rhat", 1e-12, False), ("ess_bulk", 1e-9, True),
                        ("ess_tail", 1e-9, True)):
        g, r = got[k][i], ref[k]
        if np.isnan(r):
            assert np.isnan(g), (what, k, g)
        else:
            assert abs(g - r) <= tol * (max(abs(r), 1e-300) if rel else 1.0), (what, k, g, r)


@pytest.fixture(scope="module")
def model():
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(40, 12, K=4, seed=3)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 4, device=0)
    yield m
    m.close()


def synthetic(rng, M, n, D):
    """columns of several kinds: i.i.d., AR(1), a shifted chain, integer ties, a constant, a non-finite draw"""
    x = rng.normal(size=(M, n, D))
    for i in range(1, n):
        x[:, i, 1] = 0.8 * x[:, i - 1, 1] + x[:, i, 1]
    x[0, :, 2] += 1.5
    x[:, :, 3] = rng.poisson(1.5, size=(M, n))
    x[:, :, 4] = 0.25
    x[-1, n // 3, 5] = np.nan
    return x


# (M, n): every chain count of {1, 4, 8, 64} with n in {5, 250, 251} (64 x 251 = 16 064 draws already takes the global-memory
# path), and 8 x 6000 past the LDS path. Seeds fixed;
# no column of these sits on a knife edge of the Geyer truncation (the restatement's and the kernel's sums differ in the last bits)
@pytest.mark.parametrize("M,n", [(M, n) for M in (1, 4, 8, 64) for n in (5, 250, 251)] + [(8, 6000)])
def test_synthetic_draws_match_restatement(model, M, n):
    rng = np.random.default_rng(1000 * M + n)
    x = synthetic(rng, M, n, model.D)
    f = model.fit_from_draws(x)
    try:
        cols = np.arange(8)
        got = f.summary(cols, lp=False)
        assert np.array_equal(got["column"], cols)
        for i, c in enumerate(cols):
            compare(got, i, R.summary_column(x[:, :, c]), (M, n, int(c)))
    finally:
        f.close()


def test_real_fit_all_columns_and_lp(model):
    f = model.fit_nuts(chains=4, iter=300, warmup=150, seed=5)
    try:
        got = f.summary()
        assert got["column"].size == model.D + 1 and got["column"][-1] == -1
        dr, lp = f.draws(), f.diagnostics()["lp"]
        for i in range(model.D):
            compare(got, i, R.summary_column(dr[:, :, i]), i)
        compare(got, model.D, R.summary_column(lp), "lp__")
        again = f.summary()
        for k in R.FIELDS:
            assert np.array_equal(got[k], again[k], equal_nan=True), k     # the same bits on every call
    finally:
        f.close()


def test_refusals(model):
    from ppcseq_amd import _lib
    a = model.fit_advi(output_samples=100, iter=200, seed=1)
    try:
        with pytest.raises(_lib.PpcxError, match="ADVI"):
            a.summary([0])
    finally:
        a.close()
    f = model.fit_from_draws(np.random.default_rng(0).normal(size=(2, 20, model.D)))
    try:
        with pytest.raises(_lib.PpcxError, match="out of range"):
            f.summary([model.D], lp=False)
        with pytest.raises(_lib.PpcxError, match="lp__"):
            f.summary([0], lp=True)
        assert np.isfinite(f.summary([0], lp=False)["rhat"][0])
    finally:
        f.close()


def test_do_inference_check_convergence_warns_on_a_short_fit():
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.synth import synth
    d = synth(60, 16, K=3, seed=9)
    kw = dict(how_many_posterior_draws=24, chains=4, seed=2)             # 6 kept draws per chain: too few to pass
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = do_inference(d["counts"], d["X"], d["exposure"], 3, check_convergence=True, **kw)
    msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    assert any(m.startswith("Bulk Effective Samples Size (ESS) is too low") for m in msgs), msgs
    assert any(m.startswith("Tail Effective Samples Size (ESS) is too low") for m in msgs), msgs
    conv = res.convergence
    G = d["counts"].shape[0]
    assert np.array_equal(conv["column"], np.r_[3 + G + np.arange(3), -1])
    assert np.all(conv["ess_bulk"][np.isfinite(conv["ess_bulk"])] < 400)
    with warnings.catch_warnings(record=True) as w2:
        warnings.simplefilter("always")
        plain = do_inference(d["counts"], d["X"], d["exposure"], 3, **kw)
    assert not any("Effective Samples Size" in str(x.message) or "R-hat" in str(x.message) for x in w2)
    assert plain.convergence is None
    for k in ("mean", "sd", "lower", "upper", "ppc", "slope"):
        assert np.array_equal(getattr(plain, k), getattr(res, k)), k


def test_global_path_workgroups_take_several_columns():
    """8 x 6000 draws (the global-memory path) over 210 columns: the per-workgroup slices are bounded (128 MB: 147 slices of
    this shape), so workgroup w summarises columns w, w + 147, ... in turn. Column 10 holds a NaN (its workgroup leaves it early)
    and column 157 follows it on the same workgroup. Every column must give what it gives when summarised alone."""
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(100, 12, K=4, seed=4)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 4, device=0)
    try:
        assert m.D == 210
        rng = np.random.default_rng(77)
        x = rng.normal(size=(8, 6000, m.D))
        x[:, :, 157] = np.cumsum(x[:, :, 157], axis=1) * 0.01 + x[:, :, 157]
        x[3, 100, 10] = np.nan
        f = m.fit_from_draws(x)
        try:
            full = f.summary(lp=False)
            alone = f.summary(np.arange(140, 210), lp=False)          # fewer columns than slices: one per workgroup
            for k in R.FIELDS:
                assert np.array_equal(full[k][140:], alone[k], equal_nan=True), k
            assert all(np.isnan(full[k][10]) for k in R.FIELDS)
            for c in (0, 146, 147, 157, 209):
                compare(full, c, R.summary_column(x[:, :, c]), c)
        finally:
            f.close()
    finally:
        m.close()


def test_lds_path_at_its_limit_over_two_batches():
    """64 x 128 = 8 192 draws per column, the longest the LDS path takes (128 KB of LDS per workgroup), over 2 256 columns: the
    column scratch holds 2 048 of them (128 MB), so the call runs two batches. Columns of the second batch and around the seam
    must give what they give alone and match the restatement."""
    from ppcseq_amd import _lib
    from ppcseq_amd.synth import synth
    d = synth(1100, 12, K=50, seed=5)
    m = _lib.Model(d["counts"], d["X"], d["exposure"], 50, device=0)
    try:
        assert m.D == 2256
        x = np.random.default_rng(78).normal(size=(64, 128, m.D))
        x[:5, :, 2047:2050] += 0.5                                     # a few chains apart: R-hat above 1
        f = m.fit_from_draws(x)
        try:
            full = f.summary(lp=False)
            pick = np.array([0, 1, 2046, 2047, 2048, 2049, 2255])
            alone = f.summary(pick, lp=False)
            for k in R.FIELDS:
                assert np.array_equal(full[k][pick], alone[k], equal_nan=True), k
            for c in pick:
                compare(full, c, R.summary_column(x[:, :, c]), c)
        finally:
            f.close()
    finally:
        m.close()


def test_devices_path_summarises_the_pooled_chains():
    """do_inference(devices=[0, 0], check_convergence=True): the pooled fit's alpha_sub_1 summary (no lp__) is, with the lanes
    per gene pinned, the one-device fit's, bit for bit (the pooled chains are that fit's chains)."""
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.synth import synth
    d = synth(60, 12, K=5, seed=9)
    kw = dict(chains=4, launch=(8, 0), how_many_posterior_draws=400, seed=31, check_convergence=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        one = do_inference(d["counts"], d["X"], d["exposure"], 5, **kw)
        two = do_inference(d["counts"], d["X"], d["exposure"], 5, devices=[0, 0], **kw)
    G = d["counts"].shape[0]
    assert np.array_equal(one.convergence["column"], np.r_[3 + G + np.arange(5), -1])
    assert np.array_equal(two.convergence["column"], 3 + 5 + np.arange(5))           # the pooled model holds the K checked genes
    for k in R.FIELDS:
        assert np.array_equal(one.convergence[k][:5], two.convergence[k], equal_nan=True), k


def _frame():
    import pandas as pd
    from ppcseq_amd.synth import synth
    d = synth(60, 12, K=4, seed=12)
    G, S = d["counts"].shape
    rows = [(f"s{s_:02d}", f"g{g:03d}", int(d["counts"][g, s_]), "B" if d["X"][s_, 1] else "A", g < 4, 0.5 if g < 4 else 0.9 + 1e-6 * g)
            for g in range(G) for s_ in range(S)]
    return pd.DataFrame(rows, columns=["sample", "symbol", "value", "Label", "is_significant", "PValue"]), G


def test_identify_outliers_check_convergence_attrs():
    """identify_outliers(check_convergence=True): both passes' summaries in the attrs (alpha_sub_1 of the 4 checked genes and
    lp__), the frame itself unchanged; just_discovery keeps the discovery pass's summary."""
    from ppcseq_amd.methods import identify_outliers
    data, G = _frame()
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=5, how_many_negative_controls=100,
              approximate_posterior_inference=False, approximate_posterior_analysis=False, cores=4, seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = identify_outliers(data, **kw)
        out = identify_outliers(data, check_convergence=True, **kw)
        disc = identify_outliers(data, check_convergence=True, just_discovery=True, **kw)
    assert "convergence_test" not in plain.attrs
    cols = np.r_[3 + G + np.arange(4), -1]
    for key in ("convergence_discovery", "convergence_test"):
        conv = out.attrs[key]
        assert np.array_equal(conv["column"], cols), key
        assert np.all(np.isfinite(conv["rhat"])) and np.all(conv["ess_bulk"] > 0), key
    assert not np.array_equal(out.attrs["convergence_discovery"]["mean"], out.attrs["convergence_test"]["mean"])
    assert plain["ppc_samples_failed"].tolist() == out["ppc_samples_failed"].tolist()
    for a, b in zip(plain["sample_wise_data"], out["sample_wise_data"]):
        assert np.array_equal(a[".upper"].to_numpy(), b[".upper"].to_numpy())
    assert np.array_equal(disc.attrs["convergence_discovery"]["column"], cols)
    for k in R.FIELDS:
        assert np.array_equal(disc.attrs["convergence_discovery"][k], out.attrs["convergence_discovery"][k], equal_nan=True), k
