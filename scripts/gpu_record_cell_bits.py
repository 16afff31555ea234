"""Record what a bits test (tests/test_gpu_cell_bits.py, or the module --module names: its GROUPS, evaluate, pack and GOLDEN)
compares against: every field of the per-cell entries on the test's groups, from the product and the testing build of the
commit the kernels must keep the bits of. A group that the module's RECORDED maps to another group's recording is not recorded.
Runs on the GPU.

    git worktree add ../parent <commit> && (cd ../parent && python -m ppcseq_amd.build --testing)   # the parent, in a copy of the tree
    PPCX_LIB=../parent/ppcseq_amd/libppcx.so python scripts/gpu_record_cell_bits.py --testing-lib ../parent/tests/libppcx_testing.so \
        [--module tests.test_gpu_mm_bits]

The groups and their inputs come from the test module of THIS tree; only the two libraries are the parent's."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppcseq_amd import _lib                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--testing-lib", required=True)
    ap.add_argument("--module", default="tests.test_gpu_cell_bits")
    ap.add_argument("--out", help="default: the module's GOLDEN")
    a = ap.parse_args()
    T = importlib.import_module(a.module)
    a.out = a.out or T.GOLDEN
    _lib.use_library(None)
    print("library:", _lib.LIB_PATH, "testing build:", a.testing_lib, flush=True)
    out = {}
    for group in T.GROUPS:
        if group in getattr(T, "RECORDED", {}):
            continue
        items = T.evaluate(_lib, group, a.testing_lib)
        out[group] = T.pack(items)
        print(group, len(items), "arrays", out[group].size, "values", int(np.isfinite(out[group]).sum()), "finite", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes", flush=True)


if __name__ == "__main__":
    main()
