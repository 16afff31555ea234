"""The per_sample keyword's argument checks (Model, do_inference, identify_outliers, the passes over ranks): ValueError before
anything touches a device; the C entry's own check as a status."""
import ctypes

import numpy as np
import pytest


def _inputs(S=6):
    counts = np.arange(3 * S, dtype=np.int32).reshape(3, S)
    X = np.stack([np.ones(S), (np.arange(S) % 2).astype(float)], axis=1)
    return counts, X, np.zeros(S)


@pytest.mark.parametrize("bad", ["LDS", "streamed", "", None, 1])
def test_model_refuses_other_values(bad):
    from ppcseq_amd import _lib
    counts, X, expo = _inputs()
    with pytest.raises(ValueError, match="per_sample"):
        _lib.Model(counts, X, expo, 1, per_sample=bad)


@pytest.mark.parametrize("route", ["stream", "auto"])
def test_model_refuses_a_shard_off_lds(route):
    from ppcseq_amd import _lib
    counts, X, expo = _inputs()
    with pytest.raises(ValueError, match="shard"):
        _lib.Model(counts, X, expo, 0, shard=(6, 1, 0, 3), per_sample=route)
    with pytest.raises(ValueError, match="shard"):
        _lib.Model(counts, X, expo, 0, shard=(6, 1, 0, None, 2), per_sample=route)


def test_passes_refuse_other_values():
    from ppcseq_amd import distributed, inference
    counts, X, expo = _inputs()
    with pytest.raises(ValueError, match="per_sample"):
        inference.do_inference(counts, X, expo, 1, per_sample="global")
    for route in ("stream", "auto"):             # passes over several ranks stay on LDS
        with pytest.raises(ValueError, match="per_sample"):
            distributed.do_inference(counts, X, expo, 1, per_sample=route)
        with pytest.raises(ValueError, match="per_sample"):
            distributed.do_inference_shards(counts, X, expo, 1, per_sample=route)


def test_identify_outliers_refuses_other_values():
    pd = pytest.importorskip("pandas")
    from ppcseq_amd import methods
    df = pd.DataFrame({"sample": ["a"], "transcript": ["t"], "count": [1], "PValue": [0.5], "do_check": [True]})
    with pytest.raises(ValueError, match="per_sample"):
        methods.identify_outliers(df, per_sample="global")
    with pytest.raises(ValueError, match="per_sample"):
        methods.identify_outliers(df, per_sample="stream", _pass=lambda *a, **k: None)


def test_c_entry_checks_per_sample_before_any_device_call():
    from ppcseq_amd import _lib
    lib = _lib.load()
    assert _lib.PER_SAMPLE == {"lds": 0, "stream": 1, "auto": 2}     # include/ppcx.h PPCX_PER_SAMPLE_*
    counts, X, expo = _inputs()
    h = ctypes.c_void_p(0xdead)
    rc = lib.ppcx_model_create_ex(0, 3, 6, 2, 1, _lib._p(counts, ctypes.c_int32), _lib._p(np.asfortranarray(X), ctypes.c_double),
                                  _lib._p(expo, ctypes.c_double), 5.6, 0, None, 3, ctypes.byref(h))
    assert rc == -1 and b"per_sample" in lib.ppcx_last_error() and not h.value
    rc = lib.ppcx_model_create_ex(0, 0, 6, 2, 0, None, None, None, 5.6, 0, None, 1, ctypes.byref(h))
    assert rc == -1 and b"G>=1" in lib.ppcx_last_error()
    v = ctypes.c_int()
    assert lib.ppcx_model_get_per_sample(None, ctypes.byref(v)) == -1
