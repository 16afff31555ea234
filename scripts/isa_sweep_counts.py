#!/usr/bin/env python3
"""Count the vector instructions of the log-likelihood sweep in the gfx950 ISA of its translation units (no GPU needed).

    python scripts/isa_sweep_counts.py [--asm FILE ...] [--tu NAME ...] [--keep DIR] [--kernel NAME ...] [--label TEXT]

Compiles translation units of ppcseq_amd/csrc (--tu; by default ppcx_kernels_ls.hip and ppcx_kernels.hip, which hold the default
kernels) to assembly with the flags of ppcseq_amd/build.py (--cuda-device-only -S; minutes each) -- or reads assembly files made
that way (--asm) -- and prints one JSON object: for each requested kernel

  trips     every loop block (a basic block that branches back to its own label) holding a multiple of four v_rcp_f64: its label,
            its vector instructions, how many four-cell trips it holds (v_rcp_f64 / 4) and the vector instructions per trip;
            `opcodes` says which they are
  pass      per opcode, the vector instructions of the blocks that lie between the first and the last such loop and are not
            such loops themselves (what surrounds the trips: the pass loop, the sweep variants' entries, the remainders, the
            gene sums; all seven lanes-per-gene variants of the kernel together -- a static count, not an executed one)
  variants  the same per lanes-per-gene variant of the kernel (the blocks up to and including the variant's last loop; the
            lanes are read off the stride of the loop's count loads): `cells` the vector instructions of the blocks that hold
            cells outside the loops (v_cvt_f64_u32: remainders, trips of masked passes, the odd last trip), `glue` those of all
            other blocks -- the pass loop, the sweeps' entries and exits, the gene sums and stores
  metadata  the code object's register and spill counts (vgpr_count, vgpr_spill_count, sgpr_count, sgpr_spill_count, scratch)

A vector instruction is one whose mnemonic starts with v_ (what SQ_INSTS_VALU counts); LDS and memory instructions are not.
The tool only counts opcodes: it judges nothing, and no test runs it.
"""
from __future__ import annotations

import argparse
import collections
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_KERNELS = ["ppcx_ls_kernelILi2ELi0EE", "ppcx_loglik_kernelILi2ELi0EE"]
DEFAULT_TUS = ["ppcx_kernels_ls.hip", "ppcx_kernels.hip"]      # the translation units that hold them

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
_COUNT_LOAD = re.compile(r"^\s+global_load_dword\s+v\d+, v\[\d+:\d+\], off(?: offset:(-?\d+))?\s*$")


def build_module(root: str = ROOT):
    """ppcseq_amd/build.py of the source tree `root`, loaded by path (nothing is built, the package is not imported)"""
    spec = importlib.util.spec_from_file_location("_ppcx_build_" + str(abs(hash(root))), os.path.join(root, "ppcseq_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def asm_command(out: str, tu: str, root: str = ROOT, extra=()):
    """the compiler line that turns translation unit `tu` of the tree `root` into device assembly, with that tree's own flags"""
    b = build_module(root)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-Wno-unused-result"] + b.CODEGEN_FLAGS + \
           list(extra) + ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, tu)]


def compile_asm(out: str, tu: str) -> None:
    cmd = asm_command(out, tu)
    print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)


def kernel_bodies(lines):
    """{mangled name: lines of its body} for every function of the assembly file"""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(ln)
    return out


def blocks_of(body):
    """[(label, [mnemonics], [branch targets], [offsets of its dword loads])] in the order of the text; the entry block is labelled 'entry'"""
    blocks = [("entry", [], [], [])]
    for ln in body:
        ln = ln.split(";")[0].rstrip()
        m = _LABEL.match(ln)
        if m:
            blocks.append((m.group(1), [], [], []))
            continue
        m = _INSN.match(ln)
        if not m:
            continue
        blocks[-1][1].append(m.group(1))
        c = _COUNT_LOAD.match(ln)
        if c:
            blocks[-1][3].append(int(c.group(1) or 0))
        b = _BRANCH.match(ln)
        if b:
            blocks[-1][2].append(b.group(1))
    return blocks


def _valu(ops):
    return [o for o in ops if o.startswith("v_")]


def metadata_of(lines, name):
    """the amdhsa.kernels entry of kernel `name` (the YAML at the end of the file; flat key: value pairs suffice)"""
    want = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size", "agpr_count",
            "group_segment_fixed_size")
    out, cur, start = {}, {}, False
    for ln in lines:
        if ln.strip() == "amdhsa.kernels:":
            start = True
            continue
        if not start:
            continue
        s = ln.strip()
        if s.startswith("- .") and not s.startswith("- .address_space") and not s.startswith("- .offset") and not s.startswith("- .actual_access") and ln.startswith("  - "):
            if cur.get("name") == name:
                out = cur
            cur = {}
            s = s[2:]
        m = re.match(r"^\.(\w+):\s*(\S+)$", s)
        if m and ln.startswith("    .") or (m and ln.startswith("  - .")):
            k, v = m.group(1), m.group(2)
            if k == "name":
                cur["name"] = v
            elif k in want:
                cur[k] = int(v)
    if cur.get("name") == name:
        out = cur
    out.pop("name", None)
    return out


def count_kernel(files, pattern):
    """files: [(lines, kernel_bodies(lines))], one entry per assembly file; the kernel is looked for in all of them"""
    found = [(lines, bodies, n) for lines, bodies in files for n in bodies if pattern in n]
    if len(found) != 1:
        raise SystemExit("kernel pattern %r matches %d functions: %s" % (pattern, len(found), [n for _, _, n in found]))
    lines, bodies, name = found[0]
    blocks = blocks_of(bodies[name])
    trips, idx = [], []
    for i, (label, ops, targets, offs) in enumerate(blocks):
        nr = ops.count("v_rcp_f64_e32") + ops.count("v_rcp_f64_e64") + ops.count("v_rcp_f64")
        if nr and nr % 4 == 0 and label in targets:
            v = _valu(ops)
            at = sorted(set(offs))                                  # the count loads of a trip lie L ints apart; one lane per gene
            lanes = min(b - a for a, b in zip(at, at[1:])) // 4 if len(at) > 1 else 1      # reads its four counts in one request
            trips.append({"label": label, "lanes": lanes, "valu": len(v), "trips": nr // 4, "valu_per_trip": len(v) / (nr // 4),
                          "instructions": len(ops), "opcodes": dict(sorted(collections.Counter(v).items()))})
            idx.append(i)
    between = collections.Counter()
    nblocks = 0
    if idx:
        for i in range(idx[0] + 1, idx[-1]):
            if i in idx:
                continue
            nblocks += 1
            between.update(_valu(blocks[i][1]))
    # the lanes-per-gene variants follow each other in the text, each with its loops
    variants, start = [], (idx[0] + 1 if idx else 0)
    for n, i in enumerate(idx):
        last = n + 1 == len(idx) or trips[n + 1]["lanes"] != trips[n]["lanes"]
        if not last:
            continue
        first = variants[-1]["_end"] + 1 if variants else 0
        cells = glue = 0
        for j in range(first, i):
            if j in idx:
                continue
            v = _valu(blocks[j][1])
            if "v_cvt_f64_u32_e32" in v:
                cells += len(v)
            else:
                glue += len(v)
        variants.append({"lanes": trips[n]["lanes"], "cells": cells, "glue": glue, "_end": i})
    for v in variants:
        del v["_end"]
    whole = collections.Counter(o for _, ops, _, _ in blocks for o in ops)
    return {"kernel": name, "trips": trips,
            "variants": variants,
            "pass": {"blocks": nblocks, "valu": sum(between.values()), "opcodes": dict(sorted(between.items()))},
            "whole_kernel": {"valu": sum(n for o, n in whole.items() if o.startswith("v_")), "v_readlane_b32": whole.get("v_readlane_b32", 0),
                             "v_writelane_b32": whole.get("v_writelane_b32", 0), "scratch_load": sum(n for o, n in whole.items() if o.startswith("scratch_load")),
                             "scratch_store": sum(n for o, n in whole.items() if o.startswith("scratch_store"))},
            "metadata": metadata_of(lines, name)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", action="append", help="an assembly file of a translation unit made with the library's flags; may be "
                    "repeated, the kernels are looked for in all of them (default: compile --tu)")
    ap.add_argument("--tu", action="append", help="a translation unit of ppcseq_amd/csrc to compile; may be repeated (default: %s)" % ", ".join(DEFAULT_TUS))
    ap.add_argument("--keep", help="a directory in which to leave the compiled assembly, <translation unit>.s (default: temporary files, removed)")
    ap.add_argument("--kernel", action="append", help="part of a kernel's mangled name; may be repeated (default: %s)" % ", ".join(DEFAULT_KERNELS))
    ap.add_argument("--label", default="", help="a note that travels with the output (the commit counted, for instance)")
    a = ap.parse_args()
    paths = a.asm
    with tempfile.TemporaryDirectory() as tmp:
        if paths is None:
            where = a.keep or tmp
            os.makedirs(where, exist_ok=True)
            paths = []
            for tu in a.tu or DEFAULT_TUS:          # one after the other: each takes minutes and a core
                paths.append(os.path.join(where, os.path.splitext(tu)[0] + ".s"))
                compile_asm(paths[-1], tu)
        files = []
        for path in paths:
            with open(path) as f:
                lines = f.read().splitlines()
            files.append((lines, kernel_bodies(lines)))
    out = {"label": a.label, "kernels": [count_kernel(files, k) for k in (a.kernel or DEFAULT_KERNELS)]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
