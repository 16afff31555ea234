"""ppcseq_amd/build.py: its lists agree with what is in ppcseq_amd/csrc -- every translation unit is compiled, every header a
source includes is one whose change makes a library stale, and the translation units of the log-likelihood sweep, which take
minutes, start first. Reads names and text only: nothing is compiled."""
import os
import re

from ppcseq_amd import build

SWEEP = ["ppcx_kernels.hip", "ppcx_kernels_stream.hip", "ppcx_kernels_ls.hip"]
_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]*ppcx[^"]*\.h)"', re.M)


def test_every_translation_unit_is_listed_once_and_exists():
    listed = build.SOURCES + build.TESTING_SOURCES
    assert len(set(listed)) == len(listed)
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(listed) == on_disk


def test_every_included_header_is_watched(tmp_path, monkeypatch):
    watched = {os.path.realpath(os.path.join(build.CSRC, h)) for h in build.HEADERS}
    assert all(os.path.isfile(p) for p in watched)
    seen = 0
    for f in sorted(os.listdir(build.CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        with open(os.path.join(build.CSRC, f)) as src:
            for inc in _INCLUDE.findall(src.read()):
                seen += 1
                assert os.path.realpath(os.path.join(build.CSRC, inc)) in watched, (f, inc)
    assert seen > len(build.SOURCES)             # the pattern finds the includes: at least one per translation unit
    # and the staleness check reads that list: with one header in it, a library is stale exactly when it is older than that header
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    monkeypatch.setattr(build, "SOURCES", [])
    for h in build.HEADERS:
        monkeypatch.setattr(build, "HEADERS", [h])
        t = os.path.getmtime(os.path.join(build.CSRC, h))
        os.utime(lib, (t - 10.0, t - 10.0))
        assert build._stale(str(lib)), h
        os.utime(lib, (t + 10.0, t + 10.0))
        assert not build._stale(str(lib)), h


def test_the_sweep_translation_units_start_first():
    assert build.SOURCES[:len(SWEEP)] == SWEEP
