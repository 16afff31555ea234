#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds kernel by kernel (no GPU needed).

    python scripts/isa_kernel_diff.py A B [--testing] [--tu GLOB ...] [--jobs N] [--keep-a DIR] [--keep-b DIR]

A and B are each a source tree (a directory with ppcseq_amd/build.py) or a directory of assembly files (*.s) made from one with
--cuda-device-only -S and the flags of its build.py. Of a source tree the translation units ppcseq_amd/csrc/<GLOB> (default
ppcx_kernels*.hip: the NUTS / ADVI engine's kernels) are compiled that way, --jobs compilers side by side (default 8, at most 16),
with -DPPCX_TESTING under --testing; --keep-a / --keep-b leave the assembly in a directory that can be given as A or B next time.

The kernels of each side are taken by mangled name from all of its files (kernel_bodies of isa_sweep_counts.py), so a kernel may
live in different translation units on the two sides. A device function that was not inlined (it has no descriptor) is compared
too; every translation unit that calls it holds a copy, and copies that disagree are listed per file. What depends only on a
function's position in its file is normalised away: the function index inside local labels (.LBB12_3, .Lfunc_end12, .LJTI12_0)
and inside the comments behind them (Header=BB12_3), the numbering of .Ltmp labels, the padding in front of a label's comment,
and comment-only lines. Output: one line per kernel -- `same` or `differs` for the instruction text and the kernel's .amdhsa_
descriptor block (registers, scratch, LDS, spills) together, with the part that differs -- a kernel present on one side only
reported as such, and a summary line.

The tool compares text: it searches for nothing and judges nothing, and no test runs it.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_sweep_counts import asm_command, kernel_bodies      # noqa: E402

_INDEXED = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")       # .LBB12_3 -> .LBB#_3, .Lfunc_end12 -> .Lfunc_end#
_IN_COMMENT = re.compile(r"\bBB\d+(_\d+)\b")                 # "; in Loop: Header=BB12_3 Depth=1" behind a label
_PAD = re.compile(r"\s+;")                                    # a label's comment starts at a column: the padding follows the label's width
_TMP = re.compile(r"\.Ltmp\d+\b")


def normalise(body):
    """the body without what a function's position in its file decides"""
    tmp = {}
    out = []
    for ln in body:
        s = ln.strip()
        if not s or s.startswith(";"):
            continue
        ln = _TMP.sub(lambda m: tmp.setdefault(m.group(0), ".Ltmp<%d>" % len(tmp)), ln.rstrip())
        ln = _INDEXED.sub(lambda m: ".L%s#%s" % (m.group(1), m.group(2) or ""), ln)
        ln = _IN_COMMENT.sub(lambda m: "BB#" + m.group(1), ln)
        out.append(_PAD.sub(" ;", ln))
    return out


def split_kernel(body):
    """(instruction text, descriptor block) of a kernel's body, or None for a function that is not a kernel"""
    for i, ln in enumerate(body):
        if ln.strip().startswith(".amdhsa_kernel"):
            for j in range(i, len(body)):
                if body[j].strip().startswith(".end_amdhsa_kernel"):
                    return body[:i] + body[j + 1:], body[i:j + 1]
    return None


def compile_tree(root, patterns, extra, jobs, where):
    csrc = os.path.join(root, "ppcseq_amd", "csrc")
    tus = sorted({os.path.basename(p) for pat in patterns for p in glob.glob(os.path.join(csrc, pat))})
    if not tus:
        raise SystemExit("no translation unit of %s matches %s" % (csrc, patterns))
    pending = [(tu, asm_command(os.path.join(where, os.path.splitext(tu)[0] + ".s"), tu, root, extra)) for tu in tus]
    running = []
    while pending or running:
        while pending and len(running) < jobs:
            tu, cmd = pending.pop(0)
            print(" ".join(cmd), file=sys.stderr)
            running.append((tu, subprocess.Popen(cmd)))
        tu, p = running.pop(0)
        if p.wait() != 0:
            for _, q in running:
                q.kill()
            raise SystemExit("compiling %s of %s failed" % (tu, root))


def kernels_of(side, patterns, extra, jobs, keep, tmp):
    """{mangled name: (file, text, descriptor)} of a source tree or a directory of assembly files"""
    where = side
    if os.path.exists(os.path.join(side, "ppcseq_amd", "build.py")):
        where = keep or tempfile.mkdtemp(dir=tmp)
        os.makedirs(where, exist_ok=True)
        compile_tree(side, patterns, extra, jobs, where)
    out, called = {}, {}
    for path in sorted(glob.glob(os.path.join(where, "*.s"))):
        stem = os.path.splitext(os.path.basename(path))[0]
        with open(path) as f:
            bodies = kernel_bodies(f.read().splitlines())
        for name, body in bodies.items():
            parts = split_kernel(body)
            if parts is None:                    # a device function that was not inlined: every translation unit that calls it has a copy
                called.setdefault(name, []).append((stem, normalise(body)))
                continue
            if name in out:
                raise SystemExit("%s is in %s and in %s" % (name, out[name][0], stem))
            out[name] = (stem, normalise(parts[0]), normalise(parts[1]))
    if not out:
        raise SystemExit("no kernel found in %s" % where)
    for name, copies in called.items():          # one entry if the copies agree, one per file otherwise
        if all(c[1] == copies[0][1] for c in copies):
            out[name] = ("+".join(c[0] for c in copies), copies[0][1], [])
        else:
            for fname, text in copies:
                out["%s [%s]" % (name, fname)] = (fname, text, [])
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", metavar="A", help="a source tree or a directory of assembly files")
    ap.add_argument("b", metavar="B", help="the other one")
    ap.add_argument("--testing", action="store_true", help="compile source trees with -DPPCX_TESTING")
    ap.add_argument("--tu", action="append", help="translation units of ppcseq_amd/csrc to compile, a glob; may be repeated (default: ppcx_kernels*.hip)")
    ap.add_argument("--jobs", type=int, default=8, help="compilers side by side (default 8, at most 16)")
    ap.add_argument("--keep-a", help="a directory in which to leave A's assembly")
    ap.add_argument("--keep-b", help="a directory in which to leave B's assembly")
    o = ap.parse_args()
    patterns = o.tu or ["ppcx_kernels*.hip"]
    extra = ["-DPPCX_TESTING"] if o.testing else []
    jobs = max(1, min(16, o.jobs))
    with tempfile.TemporaryDirectory() as tmp:
        ka = kernels_of(o.a, patterns, extra, jobs, o.keep_a, tmp)
        kb = kernels_of(o.b, patterns, extra, jobs, o.keep_b, tmp)
    n_same = n_diff = n_a = n_b = 0
    print("# A: %s\n# B: %s%s" % (o.a, o.b, "  (-DPPCX_TESTING)" if o.testing else ""))
    for name in sorted(set(ka) | set(kb)):
        if name not in kb:
            n_a += 1
            print("%-60s only in A (%s)" % (name, ka[name][0]))
        elif name not in ka:
            n_b += 1
            print("%-60s only in B (%s)" % (name, kb[name][0]))
        else:
            (fa, ta, da), (fb, tb, db) = ka[name], kb[name]
            where = "%s -> %s" % (fa, fb)
            if ta == tb and da == db:
                n_same += 1
                print("%-60s same     %5d lines  %s" % (name, len(ta), where))
            else:
                n_diff += 1
                what = " and ".join(w for w, d in (("instruction text", ta != tb), ("descriptor", da != db)) if d)
                print("%-60s differs  (%s)  %s" % (name, what, where))
    n_fn = sum(1 for name in set(ka) | set(kb) if not (ka.get(name) or kb[name])[2])       # no descriptor: a called function
    print("# %d kernels and %d called functions: %d same, %d differ, %d only in A, %d only in B"
          % (n_same + n_diff + n_a + n_b - n_fn, n_fn, n_same, n_diff, n_a, n_b))


if __name__ == "__main__":
    main()
