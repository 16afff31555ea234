"""Record what tests/test_gpu_sweep_bits.py compares against: lp, gradients and a short fit of the test's cases, from the build
of the commit the sweep must keep the bits of. Runs on the GPU.

    git worktree add ../parent <commit> && (cd ../parent && python -m ppcseq_amd.build)        # the parent, in a copy of the tree
    PPCX_LIB=../parent/ppcseq_amd/libppcx.so python scripts/gpu_record_sweep_bits.py --out tests/golden/sweep_bits_parent.npz

The cases come from the test module of THIS tree; only the library is the parent's (PPCX_LIB)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppcseq_amd import _lib                                  # noqa: E402
from tests import test_gpu_sweep_bits as T                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    _lib.use_library(None)
    print("library:", _lib.LIB_PATH, flush=True)
    groups = {}
    for key, variant, S, lanes, n in T.calls():
        groups.setdefault((variant, S, n), []).append((key, lanes))
    per_key = {}
    for (variant, S, n), keyed in sorted(groups.items()):
        got = T.evaluate(_lib, variant, S, [lanes for _, lanes in keyed], n)
        for key, lanes in keyed:
            lp, g = got[lanes]
            assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)), key
            per_key[key] = (lp, g)
        print(variant, S, n, "lp[0] per lanes:", [float(got[lanes][0][0]) for _, lanes in keyed], flush=True)
    out = T.pack(per_key)
    out.update(T.short_fit(_lib))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes", flush=True)


if __name__ == "__main__":
    main()
