"""The split transformation of gene-local moment matching on the device (Fit.loo_moment_match(split=True),
Fit.loo_predict_exact_moment_match(split=True); ppcx_fit_loo_moment_match_split, ppcx_fit_loo_predict_exact_moment_match_split):
the designed draws of tests/loo_mm_cases.py reach the kernel through Model.fit_from_draws and are held to the CPU build of its
header (tests/loo_mm_split_twin); the draw counts at the wavefront, the workgroup's stride, h = n / 2 on a stride boundary and
the LDS / scratch hand-over, with the scratch in batches of two cells (testing build); the truth case; and a short NUTS fit of
the bundled case: the same bits on every call, split=False against the method without the keyword, the refusal of an ADVI fit
and identify_outliers with the two flags.

Both entries are asked of one fit, and the predictive one takes checked genes only: checked_all() of
tests/test_gpu_loo_mm_exact.py gives every gene a slope column, and the CPU build reads the same gene.

Tolerances: iterations equal, NaN and Inf in the same places; what the split leaves alone -- khat, khat_before, iterations,
scale, shift, y, excluded, and elpd_loo_matched against the unsplit elpd_loo -- bit-equal to the unsplit entry, a cell with
iterations == 0 in full; the rest against the CPU build at ten times the largest error measured on the designed cells, the draw
counts and the truth case in units of max(1, |ref|), p_le / p_ge also relatively below 1e-3 (S.GPU_MEASURED; the tests print
theirs), never above 1e-9."""
import numpy as np
import pytest

from tests import loo_mm_cases as cases
from tests import loo_mm_exact_restate as X
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as S
from tests.conftest import bundled_test_config
from tests.gpu_fixtures import testing_library
from tests.test_gpu_loo_mm_exact import _Held, _against_host as _exact_against_host, checked_all
from tests.test_gpu_psis import _bundled_frame

pytestmark = pytest.mark.gpu

GPU_BOUND = min(10 * S.GPU_MEASURED, S.BOUND)
TC = 0.7352941
MM_KEPT = ("khat", "khat_before", "iterations", "scale", "shift")            # the matching's bits in both split records
KEYS = R.HEAD + ("scale", "shift") + S.TAIL
XKEYS = X.HEAD + ("scale", "shift", "khat_split", "pit_lt", "pit_le")


@pytest.fixture(scope="module")
def host():
    return S.host_lib()


def _row(res, i, s):
    return np.concatenate([[res[k][i, s] for k in R.HEAD], res["scale"][i, s], res["shift"][i, s], [res[k][i, s] for k in S.TAIL]]).astype(np.float64)


def _against_host(got, ref, what):
    """the elpd form's cell against the CPU build's record: iterations and the places of NaN / Inf equal; the error of the rest"""
    assert got[5] == ref[5], (what, got[5], ref[5])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), (what, got, ref)
    return max(S._err(g, r) for j, (g, r) in enumerate(zip(got, ref)) if j != 5)


def _exact_against(res, i, s, ref, what):
    """the predictive form's cell against the CPU build's record (tests/test_gpu_loo_mm_exact.py's comparison, and khat_split)"""
    ks = res["khat_split"][i, s]
    assert np.isnan(ks) == np.isnan(ref[-1]), (what, ks, ref[-1])
    return max(_exact_against_host(res, i, s, ref[:-1], what), S._err(ks, ref[-1]))


def _both(fit, genes, **kw):
    """the four records of the same cells: elpd form split / unsplit, predictive form split / unsplit"""
    xkw = dict(kw, truncation_compensation=TC)
    return (fit.loo_moment_match(genes, split=True, **kw), fit.loo_moment_match(genes, **kw),
            fit.loo_predict_exact_moment_match(genes, split=True, **xkw), fit.loo_predict_exact_moment_match(genes, **xkw))


def _kept_bits(res, un, xres, xun, what):
    """what the split leaves alone is the unsplit entry's bits; a cell with iterations == 0 in full"""
    it = un["iterations"]
    assert np.array_equal(res["iterations"], it) and np.array_equal(xres["iterations"], it), what
    for k in MM_KEPT:
        assert np.array_equal(res[k], un[k], equal_nan=True), (what, k)
    assert np.array_equal(res["elpd_loo_matched"], un["elpd_loo"], equal_nan=True), what
    for k in ("y", "excluded", "khat_before", "scale", "shift"):
        assert np.array_equal(xres[k], xun[k], equal_nan=True), (what, k)
    ok = ~np.isnan(xres["mean"])
    assert np.array_equal(xres["khat"][ok], xun["khat"][ok], equal_nan=True), what     # the matching's final k
    for k in R.HEAD:
        assert np.array_equal(res[k][it == 0], un[k][it == 0], equal_nan=True), (what, k)
    for k in X.HEAD + ("pit_lt", "pit_le"):
        assert np.array_equal(xres[k][it == 0], xun[k][it == 0], equal_nan=True), (what, k)
    assert np.all(np.isnan(res["khat_split"][it == 0])) and np.all(np.isnan(xres["khat_split"][it == 0])), what
    assert np.array_equal(res["khat_split"][ok], xres["khat_split"][ok], equal_nan=True), what      # PSIS on the same ratios


def test_designed_cells_against_the_cpu_build(host):
    held, sets = {}, {}
    worst, split = 0.0, 0
    try:
        for c in cases.designed():
            if c["set"] not in held:
                sets[c["set"]] = checked_all(cases.draw_set(c["set"]))
                held[c["set"]] = _Held(sets[c["set"]])
            ds, fit = sets[c["set"]], held[c["set"]].fit
            S_ = ds["counts"].shape[1]
            kw = dict(k_threshold=c["k_threshold"], max_iters=c["max_iters"])
            res, un, xres, xun = _both(fit, [c["g"]], r_eff=np.full((1, S_), c["r_eff"]), **kw)
            assert res["khat_split"].shape == (1, S_) and res["iterations"].dtype == np.int64 and xres["scale"].shape == (1, S_, 3)
            _kept_bits(res, un, xres, xun, c["name"])
            gene = cases.gene_of(ds, c["g"])
            for s in range(S_):                                           # the designed cell and its gene's other cells
                ref = S.host_cell(host, gene, s, r_eff=c["r_eff"], **kw)
                xref = S.host_exact_cell(host, gene, s, r_eff=c["r_eff"], tc=TC, **kw)
                err = _against_host(_row(res, 0, s), ref, (c["name"], s))
                xerr = _exact_against(xres, 0, s, xref, (c["name"], s))
                worst = max(worst, err, xerr)
                assert err <= GPU_BOUND and xerr <= GPU_BOUND, (c["name"], s, err, xerr)
                split += ref[5] > 0
    finally:
        for h in held.values():
            h.close()
    print("cells split", int(split), "largest error against the CPU build:", worst)
    assert split >= 8
    assert worst <= S.GPU_MEASURED                                    # the recorded value is the measured one


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097])
def test_draw_counts(host, n):
    """the wavefront, the workgroup's stride, h on a stride boundary (n = 512) and the LDS / scratch hand-over; the scratch bound
    set so that the scratch path runs in batches of two cells (and the gene table in batches of two genes)"""
    ds = cases.prefix(checked_all(cases.long_set()), n)
    with testing_library() as _lib:
        h = _Held(ds)
        try:
            one = h.fit.loo_moment_match(k_threshold=0.7, split=True)     # (loo_threshold is not defined at one draw)
            xone = h.fit.loo_predict_exact_moment_match(k_threshold=0.7, split=True, truncation_compensation=TC)
            _lib.testing_set("loo_scratch_bytes", 2 * 8 * 3 * n + 8)
            try:
                res, un, xres, xun = _both(h.fit, np.arange(2), k_threshold=0.7)
            finally:
                _lib.testing_set("loo_scratch_bytes", 0)
        finally:
            h.close()
    for k in KEYS:
        assert np.array_equal(res[k], one[k], equal_nan=True), k       # the same bits however the work is batched
    for k in XKEYS:
        assert np.array_equal(xres[k], xone[k], equal_nan=True), k
    _kept_bits(res, un, xres, xun, n)
    split, worst = 0, 0.0
    for g in range(2):
        gene = cases.gene_of(ds, g)
        for s in range(4):
            ref = S.host_cell(host, gene, s, k_threshold=0.7)
            xref = S.host_exact_cell(host, gene, s, k_threshold=0.7, tc=TC)
            err = _against_host(_row(res, g, s), ref, (n, g, s))
            xerr = _exact_against(xres, g, s, xref, (n, g, s))
            worst = max(worst, err, xerr)
            assert err <= GPU_BOUND and xerr <= GPU_BOUND, (n, g, s, err, xerr)
            split += res["iterations"][g, s] > 0
    print("n", n, "cells split", int(split), "largest error against the CPU build", worst)
    assert split >= (1 if n >= 63 else 0)
    assert worst <= S.GPU_MEASURED


def test_truth_case(host):
    """n = 1000, seed 1: the device gives the CPU build's figures (tests/test_loo_mm_split_host.py holds those to the truth)"""
    ds = checked_all(cases.truth_set(1, 1000))
    h = _Held(ds)
    try:
        res, un, xres, xun = _both(h.fit, [0])
    finally:
        h.close()
    _kept_bits(res, un, xres, xun, "truth")
    s = cases.TRUTH_CELL
    gene = cases.gene_of(ds, 0)
    ref, xref = S.host_cell(host, gene, s), S.host_exact_cell(host, gene, s, tc=TC)
    err = _against_host(_row(res, 0, s), ref, "truth")
    xerr = _exact_against(xres, 0, s, xref, "truth")
    truth = cases.truth_elpd()
    print("truth case: khat", res["khat"][0, s], "khat_split", res["khat_split"][0, s], "|elpd_loo - truth| matched",
          abs(res["elpd_loo_matched"][0, s] - truth), "split", abs(res["elpd_loo"][0, s] - truth), "upper", xun["upper"][0, s], "->",
          xres["upper"][0, s], "errors against the CPU build", err, xerr)
    assert err <= GPU_BOUND and xerr <= GPU_BOUND and ref[5] == 2
    assert abs(res["elpd_loo"][0, s] - truth) < abs(res["elpd_loo_matched"][0, s] - truth)
    assert max(err, xerr) <= S.GPU_MEASURED                           # the recorded value is the measured one


EXCL = (0 * 21 + 3, 2 * 21 + 20)                     # the two cells the model holds out


@pytest.fixture(scope="module")
def fits(bundled):
    from ppcseq_amd import _lib
    counts, X_, _, K = bundled_test_config(bundled)
    libsize = np.log(counts.sum(axis=0).astype(np.float64))
    expo = libsize.mean() - libsize
    m = _lib.Model(counts, X_, expo, K, excl=np.array(EXCL, np.int32), device=0)
    nuts = m.fit_nuts(chains=3, iter=300, warmup=150, seed=7)
    advi = m.fit_advi(output_samples=300, iter=2000, seed=4)
    yield dict(m=m, counts=counts, K=K, nuts=nuts, advi=advi)
    nuts.close()
    advi.close()
    m.close()


def test_nuts_fit(fits):
    """the bundled 53 x 21 case, 3 chains x 150 kept draws, two cells held out"""
    from ppcseq_amd import _lib
    fit, K = fits["nuts"], fits["K"]
    G, S_ = fits["counts"].shape
    full, un = fit.loo_moment_match(split=True), fit.loo_moment_match()
    xfull, xun = fit.loo_predict_exact_moment_match(split=True), fit.loo_predict_exact_moment_match()
    assert full["n_draws"] == 450 and full["khat_split"].shape == (G, S_) and xfull["khat_split"].shape == (K, S_)
    _kept_bits(fit.loo_moment_match(np.arange(K), split=True), fit.loo_moment_match(np.arange(K)), xfull, xun, "nuts")
    it = full["iterations"]
    for k in MM_KEPT:
        assert np.array_equal(full[k], un[k], equal_nan=True), k
    assert np.array_equal(full["elpd_loo_matched"], un["elpd_loo"], equal_nan=True)
    for k in R.HEAD:
        assert np.array_equal(full[k][it == 0], un[k][it == 0], equal_nan=True), k
    assert np.all(np.isnan(full["khat_split"][it == 0])) and np.all(np.isfinite(full["khat_split"][it > 0]))
    assert np.all(np.isfinite(full["elpd_loo"])) and np.array_equal(full["khat_split"][:K], xfull["khat_split"], equal_nan=True)
    changed = full["elpd_loo"][it > 0] != un["elpd_loo"][it > 0]
    print("cells split", int((it > 0).sum()), "of", it.size, "elpd_loo changed in", int(changed.sum()), "khat_split above 0.7 in",
          int((full["khat_split"][it > 0] > 0.7).sum()), "estimates", full["estimates"]["elpd_loo"], "unsplit", un["estimates"]["elpd_loo"])
    assert (it > 0).sum() >= 1 and changed.all()
    # the same bits on a second call, for a gene subset and for a permuted gene list
    again, xagain = fit.loo_moment_match(split=True), fit.loo_predict_exact_moment_match(split=True)
    perm = np.random.default_rng(3).permutation(G)
    permuted, xperm = fit.loo_moment_match(perm, split=True), fit.loo_predict_exact_moment_match(np.arange(K)[::-1], split=True)
    sub, xsub = fit.loo_moment_match([40, 7, 0], split=True), fit.loo_predict_exact_moment_match([K - 1], split=True)
    for k in KEYS:
        assert np.array_equal(again[k], full[k], equal_nan=True), k
        assert np.array_equal(permuted[k], full[k][perm], equal_nan=True), k
        assert np.array_equal(sub[k], full[k][[40, 7, 0]], equal_nan=True), k
    for k in XKEYS:
        assert np.array_equal(xagain[k], xfull[k], equal_nan=True), k
        assert np.array_equal(xperm[k], xfull[k][::-1], equal_nan=True), k
        assert np.array_equal(xsub[k], xfull[k][[K - 1]], equal_nan=True), k
    # r_eff = "auto": the matching's record is that of the unsplit entry under the same r_eff
    auto, auto_un = fit.loo_moment_match(np.arange(K), r_eff="auto", split=True), fit.loo_moment_match(np.arange(K), r_eff="auto")
    xauto = fit.loo_predict_exact_moment_match(r_eff="auto", split=True)
    assert auto["r_eff"].shape == (K, S_) and np.array_equal(auto["r_eff"], auto_un["r_eff"]) and np.array_equal(auto["r_eff"], xauto["r_eff"])
    for k in MM_KEPT:
        assert np.array_equal(auto[k], auto_un[k], equal_nan=True), k
    assert np.array_equal(auto["khat_split"], xauto["khat_split"], equal_nan=True)
    # split=False is the method without the keyword, bit for bit and key for key
    off, xoff = fit.loo_moment_match(split=False), fit.loo_predict_exact_moment_match(split=False)
    for got, ref in ((off, un), (xoff, xun)):
        assert list(got) == list(ref) and "khat_split" not in got
        for k in ref:
            if isinstance(ref[k], np.ndarray):
                assert np.array_equal(got[k], ref[k], equal_nan=True), k
            else:
                assert got[k] == ref[k], k
    # refusals
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_moment_match_split needs the draws of a NUTS fit.*ADVI fit"):
        fits["advi"].loo_moment_match(split=True)
    with pytest.raises(_lib.PpcxError, match="ppcx_fit_loo_predict_exact_moment_match_split needs the draws of a NUTS fit.*ADVI fit"):
        fits["advi"].loo_predict_exact_moment_match(split=True)
    with pytest.raises(_lib.PpcxError, match="k_threshold must be finite"):
        fit.loo_moment_match([0], k_threshold=np.nan, split=True)
    with pytest.raises(_lib.PpcxError, match="max_iters must be >= 0"):
        fit.loo_predict_exact_moment_match([0], max_iters=-1, split=True)
    with pytest.raises(_lib.PpcxError, match="gene out of range \\(a checked gene"):
        fit.loo_predict_exact_moment_match([K], split=True)


def test_identify_outliers_with_the_flags(bundled):
    """a short NUTS run of the bundled 53 x 21 case: flags and frame are those of the call without the two flags, the attrs gain
    khat_split; how many cells were split is printed, not asserted"""
    import warnings
    from ppcseq_amd.methods import identify_outliers
    df = _bundled_frame(bundled)
    kw = dict(formula="~ Label", sample="sample", transcript="symbol", abundance="value", significance="PValue",
              do_check="is_significant", percent_false_positive_genes=1, approximate_posterior_inference=False,
              approximate_posterior_analysis=False, how_many_negative_controls=50, cores=1, seed=11,
              adj_prob_theshold_2=0.01,                     # 1 000 draws in the second pass too: the test stays short
              check_loo=True, loo_moment_match=True, exact_loo_intervals=True, exact_loo_moment_match=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = identify_outliers(df, **kw)
        out = identify_outliers(df, loo_moment_match_split=True, exact_loo_moment_match_split=True, **kw)
    assert set(out.attrs) == set(plain.attrs)
    for col in plain.columns:
        assert repr(plain[col].tolist()) == repr(out[col].tolist()), col
    for key in ("loo_discovery", "loo_test", "exact_loo_intervals_discovery", "exact_loo_intervals_test"):
        r, p = out.attrs[key], plain.attrs[key]
        assert "khat_split" in r and "khat_split" not in p and r["khat_split"].shape == (3, 21), key
        for k in MM_KEPT[1:]:
            assert np.array_equal(r[k], p[k], equal_nan=True), (key, k)
        it = r["iterations"]
        assert np.all(np.isnan(r["khat_split"][it == 0]))
        if key.startswith("loo_"):
            assert np.array_equal(r["elpd_loo_matched"], p["elpd_loo"], equal_nan=True) and np.array_equal(r["khat"], p["khat"], equal_nan=True)
        print(key, "draws", r["n_draws"], "cells split", int((it > 0).sum()), "khat_split above the threshold",
              int((r["khat_split"][it > 0] > r["k_threshold"]).sum()))
    with pytest.raises(ValueError, match="^loo_moment_match_split needs loo_moment_match"):
        identify_outliers(df, **dict(kw, loo_moment_match=False, loo_moment_match_split=True))
