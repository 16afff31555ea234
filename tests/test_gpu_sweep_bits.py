"""The log-likelihood sweep keeps its bits: lp and the whole gradient of Model.log_prob_grad at pinned lanes per gene, and a short
two-chain NUTS fit, equal bit for bit to what the commit before the sweep's glue was trimmed (operand addressing, trip unrolling,
uniform bases: ppcx_gene.h sweep_cells, ppcx_loglik.h loglik_passes) returned on an MI355X. The recording is
tests/golden/sweep_bits_parent.npz, written by scripts/gpu_record_sweep_bits.py from the cases below.

Cases (the smallest shapes at which that code can go wrong): G = 70 genes, K = 3 of them with a slope, so that no pass is full and
a wavefront's range ends inside a pass; S = 200 (trips and a one- or two-cell remainder), 64 (no remainder at 1 .. 16 lanes),
37 (lanes with unequal numbers of cells, odd S), 7 (no full trip at all). Three positions per call -- a three-chain launch: one
in the typical set (intercepts near 5, sigma_raw near 0: windowed passes), one at the data's own parameters, one with sigma_raw = 9
(outside the dispersion tables: disp_row_at) -- and one call with eight.
  base     every S at 1, 4, 8, 16 and 64 lanes per gene
  wide     exposures a factor 20 apart: no gene has a window, the general cell runs
  masked   two genes with excluded cells: a masked pass in the same launch as unmasked ones
The two variants run at every S with 4 and 8 lanes per gene (the lanes the fits launch with), and with 1, 16 and 64 lanes at S = 200
and S = 37 (whole trips in pairs and an odd one, a remainder, unequal lanes; at 64 lanes one gene per pass: a masked pass between
unmasked ones in one wavefront): every lane count's loops are compared, and the recording stays below 200 KB.
The fit: two chains, 40 iterations (4 kept) at S = 37 with the automatic launch -- the merged launch of a pipelined round
(ppcx_ls_kernel)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_bits_parent.npz")
G, K = 70, 3
SIZES = (200, 64, 37, 7)
LANES = (1, 4, 8, 16, 64)
VARIANT_LANES_EVERY_S = (4, 8)
VARIANT_SIZES_EVERY_LANES = (200, 37)
FIT = dict(chains=2, iter=40, warmup=36, seed=7)
FIT_S = 37


def data(S, variant):
    """(counts, X, exposure, excluded cells) of a variant at S samples"""
    from ppcseq_amd.synth import synth
    d = synth(G, S, K=K, seed=20260 + S)
    expo = d["exposure"].copy()
    excl = None
    if variant == "wide":
        expo = np.linspace(-0.5, 0.5, S) * np.log(20.0)
        expo -= expo.mean()
    if variant == "masked":
        # a gene with a slope and a plain one; first, last and a middle cell, so that every lane count loses one somewhere
        cells = sorted({0, S // 2, S - 1})
        excl = np.array([1 * S + s for s in cells] + [40 * S + s for s in cells[:2]], np.int32)
    return d["counts"], d["X"], expo, excl, d["truth"]


def positions(S, truth, n):
    """n unconstrained positions: typical set, the data's own parameters, sigma_raw = 9, then perturbations of the first"""
    from oracle import independent as ind
    o = ind.offsets(G, 2, K)
    rng = np.random.default_rng(77 + S)
    u0 = rng.uniform(-0.3, 0.3, o["D"])
    u0[o["intercept"]:o["intercept"] + G] += 5.0
    u1 = rng.uniform(-0.1, 0.1, o["D"])
    u1[o["intercept"]:o["intercept"] + G] = truth["intercept"]
    u1[o["alpha1"]:o["alpha1"] + K] = truth["alpha"][1, :K]
    u1[o["sigma_raw"]:o["sigma_raw"] + G] = truth["sigma_raw"]
    u2 = u0.copy()
    u2[o["sigma_raw"]:o["sigma_raw"] + G] = 9.0
    U = [u0, u1, u2]
    while len(U) < n:
        U.append(u0 + rng.uniform(-0.2, 0.2, o["D"]))
    return np.array(U[:n])


def calls():
    """(key, variant, S, lanes per gene, positions per call) of every recorded call"""
    out = [("base_S%d_L%d" % (S, L), "base", S, L, 3) for S in SIZES for L in LANES]
    out.append(("base8_S200_L8", "base", 200, 8, 8))
    for variant in ("wide", "masked"):
        out += [("%s_S%d_L%d" % (variant, S, L), variant, S, L, 3) for S in SIZES for L in LANES
                if L in VARIANT_LANES_EVERY_S or S in VARIANT_SIZES_EVERY_LANES]
    return out


def evaluate(lib, variant, S, lanes_list, n):
    """{lanes: (lp, grad)} of one model at each pinned lanes-per-gene value"""
    counts, X, expo, excl, truth = data(S, variant)
    U = positions(S, truth, n)
    m = lib.Model(counts, X, expo, K, excl=excl)
    try:
        out = {}
        for lanes in lanes_list:
            m.set_launch(lanes, 0)
            out[lanes] = m.log_prob_grad(U)
        return out
    finally:
        m.close()


def short_fit(lib):
    counts, X, expo, excl, _ = data(FIT_S, "base")
    m = lib.Model(counts, X, expo, K, excl=excl)
    try:
        f = m.fit_nuts(**FIT)
        try:
            out = {"fit_draws": f.draws()}
            for k, v in f.diagnostics().items():
                out["fit_" + k] = v
            return out
        finally:
            f.close()
    finally:
        m.close()


@pytest.fixture(scope="module")
def lib():
    from ppcseq_amd import _lib
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the product has no CPU fallback")
    return _lib


def pack(per_key):
    """the calls' (lp, grad) as three arrays (one archive member per call would cost the file a tenth of its size in headers):
    the calls' keys in the order of calls(), their lp end to end, their gradients row after row"""
    keys = [c[0] for c in calls()]
    return {"keys": np.array(keys), "lp": np.concatenate([per_key[k][0] for k in keys]), "grad": np.concatenate([per_key[k][1] for k in keys])}


def unpack(z):
    out, r = {}, 0
    n_of = {c[0]: c[4] for c in calls()}
    for k in (str(k) for k in z["keys"]):
        out[k + "_lp"], out[k + "_grad"] = z["lp"][r:r + n_of[k]], z["grad"][r:r + n_of[k]]
        r += n_of[k]
    assert r == z["lp"].shape[0] == z["grad"].shape[0]
    return out


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)
    out = {k: z[k] for k in z.files if k.startswith("fit_")}
    out.update(unpack(z))
    return out


def _groups():
    seen = {}
    for key, variant, S, lanes, n in calls():
        seen.setdefault((variant, S, n), []).append((key, lanes))
    return sorted(seen.items())


@pytest.mark.parametrize("group", _groups(), ids=lambda g: "%s-S%d-n%d" % g[0])
def test_log_prob_grad_bits(lib, golden, group):
    (variant, S, n), keyed = group
    got = evaluate(lib, variant, S, [lanes for _, lanes in keyed], n)
    for key, lanes in keyed:
        lp, g = got[lanes]
        assert lp.shape == (n,) and np.all(np.isfinite(lp)), (key, lp)
        assert np.array_equal(lp, golden[key + "_lp"]), (key, lp, golden[key + "_lp"])
        bad = np.argwhere(g != golden[key + "_grad"])
        assert np.array_equal(g, golden[key + "_grad"]), (key, len(bad), bad[:5].tolist())


def test_short_fit_bits(lib, golden):
    got = short_fit(lib)
    assert got["fit_draws"].shape == (FIT["chains"], FIT["iter"] - FIT["warmup"], 3 + G + K + G + 3)
    for k, v in got.items():
        assert v.dtype == golden[k].dtype and np.array_equal(v, golden[k]), k
