"""tests/host_build.py: the dependency lists that decide whether a CPU build of the kernel headers is stale are the compiler's
and hold the headers each program really includes, and a library is rebuilt exactly when it is missing or older than one of
them (on a toy program in tmp_path: nothing in the tree is touched)."""
import os

import pytest

from tests import host_build

# the headers of ppcseq_amd/csrc that each program must depend on: the one it is named after and those that hand-written lists
# have missed
EXPECT = {
    "psis": ("ppcx_math.h", "ppcx_psis.h"),
    "summary": ("ppcx_math.h", "ppcx_summary.h"),
    "reff": ("ppcx_summary.h", "ppcx_reff.h"),
    "loo": ("ppcx_psis.h", "ppcx_summary.h", "ppcx_loo.h"),
    "loo_mcse": ("ppcx_psis.h", "ppcx_summary.h", "ppcx_loo.h"),
    "loo_predict": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_loo.h", "ppcx_loo_predict.h"),
    "loo_ap": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_loo_predict.h", "ppcx_loo_ap.h"),
    "ppc_exact": ("ppcx_nbcdf.h", "ppcx_ppc_exact.h"),
    "loo_exact": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_nbcdf.h", "ppcx_ppc_exact.h", "ppcx_loo_exact.h"),
    "loo_mm": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_ppc_exact.h", "ppcx_nbcdf.h", "ppcx_model.h", "ppcx_loo_mm.h"),
    "loo_mm_exact": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_loo_mm.h", "ppcx_loo_mm_exact.h"),
    "loo_mm_split_twin": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_loo_mm.h", "ppcx_loo_mm_exact.h", "ppcx_loo_mm_split.h"),
    "loo_mm_cov_twin": ("ppcx_summary.h", "ppcx_ppc.h", "ppcx_loo_mm.h", "ppcx_loo_mm_split.h", "ppcx_loo_mm_cov.h"),
}


def test_every_program_is_listed():
    assert sorted(EXPECT) == sorted(host_build.NAMES)
    on_disk = sorted(d[:-len("_host")] if d.endswith("_host") else d for d in os.listdir(os.path.join(host_build.ROOT, "tests"))
                     if d.endswith(("_host", "_twin")) and d != "c_host" and os.path.isdir(os.path.join(host_build.ROOT, "tests", d)))
    assert on_disk == sorted(host_build.NAMES)


@pytest.mark.parametrize("name", host_build.NAMES)
def test_dependencies_hold_the_headers_the_program_includes(name):
    src = host_build.source(name)
    deps = host_build.dependencies(src)
    assert src in deps
    csrc = os.path.join(host_build.ROOT, "ppcseq_amd", "csrc")
    for h in EXPECT[name]:
        assert os.path.join(csrc, h) in deps, (name, h, deps)
    assert all(os.path.isabs(p) and os.path.exists(p) for p in deps)


def test_rebuilds_exactly_when_stale(tmp_path):
    here = tmp_path / "tests" / "toy_host"
    here.mkdir(parents=True)
    (here / "b.h").write_text("inline int toy_b() { return 41; }\n")
    (here / "a.h").write_text('#include "b.h"\ninline int toy_a() { return toy_b() + 1; }\n')
    (here / "toy_host.cpp").write_text('#include "a.h"\nextern "C" __attribute__((visibility("default"))) int toy() { return toy_a(); }\n')
    src, lib = str(here / "toy_host.cpp"), str(here / "libtoy_host.so")
    assert sorted(host_build.dependencies(src)) == sorted([src, str(here / "a.h"), str(here / "b.h")])
    h = host_build.host_lib("toy", {"toy": ([], host_build.ctypes.c_int)}, root=str(tmp_path))
    assert h.toy() == 42
    first = os.stat(lib).st_mtime_ns
    host_build.host_lib("toy", {}, root=str(tmp_path))
    assert os.stat(lib).st_mtime_ns == first and not host_build.build(src, lib)              # built twice: compiled once
    ahead = os.stat(lib).st_mtime + 10.0
    os.utime(here / "b.h", (ahead, ahead))                       # a header that only a.h names
    assert host_build.build(src, lib) and os.stat(lib).st_mtime_ns > first
    os.utime(here / "b.h", (ahead - 20.0, ahead - 20.0))
    assert not host_build.build(src, lib)
    os.remove(lib)
    assert host_build.build(src, lib) and os.path.exists(lib)
    assert not [p for p in os.listdir(here) if p.endswith(".d")]                             # no dependency file is left
