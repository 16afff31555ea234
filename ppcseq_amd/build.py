"""Build the HIP C-ABI library (libppcx.so) in-tree with hipcc for gfx950."""
from __future__ import annotations

import os
import subprocess
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libppcx.so")
# the testing build (-DPPCX_TESTING: fault injection, forced cell paths, kernel-level timing; csrc/ppcx_testing.h) lives
# with the tests, not in the package
TESTING_LIB = os.path.join(os.path.dirname(HERE), "tests", "libppcx_testing.so")
# the three translation units of the log-likelihood sweep first (LDS-staged, streamed, merged launch): they take minutes, the
# others seconds, and the compilers start in this order
SOURCES = ["ppcx_kernels.hip", "ppcx_kernels_stream.hip", "ppcx_kernels_ls.hip",
           "ppcx_kernels_close.hip", "ppcx_kernels_model.hip", "ppcx_summary.hip", "ppcx_psis.hip", "ppcx_loo.hip", "ppcx_loo_predict.hip", "ppcx_reff.hip", "ppcx_ppc_exact.hip", "ppcx_loo_exact.hip", "ppcx_loo_mm.hip", "ppcx_loo_mm_exact.hip", "ppcx_loo_mm_split.hip", "ppcx_loo_mm_cov.hip", "ppcx_loo_mm_cov_exact.hip", "ppcx_ppc.hip",
           "ppcx_capi.hip", "ppcx_run.hip", "ppcx_fit_nuts.hip", "ppcx_fit_advi.hip", "ppcx_fit_api.hip"]
TESTING_SOURCES = ["ppcx_testing_math.hip"]      # the device's building blocks one by one (csrc/ppcx_testing.h): testing build only
# every header present, so that a new one cannot be forgotten (a stale library that looks fresh)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "ppcx.h")]


# hipcc (ROCm 7.2) miscompiles the scalar state machine of ppcx_step_kernel when the SLP vectoriser has made <2 x i32> phis of
# adjacent Cmd fields and AMDGPUCodeGenPrepare breaks them up again: the IR stays correct, the ISA loses a copy on one
# predecessor path (Cmd::rng_c3 = 0 on the halving / doubling path of the step-size search). Traced in round 4 (DESIGN.md
# section 3, profiles/r04_miscompile/): of 15 builds with single passes switched off only -fno-slp-vectorize and
# -mllvm -amdgpu-codegenprepare-break-large-phis=false give correct code. Neither changes a fit's time; the second costs
# ppcx_step_kernel nine vector registers and with them its third workgroup per CU (169 instead of 160; 158 without SLP),
# so the library is built without SLP vectorisation (scalar fp64 kernels: there is nothing for it to vectorise usefully).
CODEGEN_FLAGS = ["-fno-slp-vectorize"]


def _sources(extra):
    return SOURCES + (TESTING_SOURCES if "-DPPCX_TESTING" in extra else [])


def _stale(lib: str, extra=()) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in _sources(extra) + HEADERS)


# at most 16 compilers at a time in this process, however many builds run side by side (build_all)
_COMPILERS = threading.BoundedSemaphore(16)


def _start_compiler(cmd):
    _COMPILERS.acquire()                         # released when this compiler ends
    p = subprocess.Popen(cmd)
    threading.Thread(target=lambda: (p.wait(), _COMPILERS.release()), daemon=True).start()
    return p


def _compile(lib: str, extra, verbose: bool) -> None:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    for s in _sources(extra):                    # the translation units side by side
        o = lib + "." + s + ".o"
        objs.append(o)
        cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-Wno-unused-result"] + CODEGEN_FLAGS + extra + \
              ["-c", "-o", o, os.path.join(CSRC, s)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append(_start_compiler(cmd))
    for p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, p.args)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    for o in objs:
        os.remove(o)


def build(force: bool = False, verbose: bool = False) -> str:
    if force or _stale(LIB):
        _compile(LIB, [], verbose)
    return LIB


def build_testing(force: bool = False, verbose: bool = False) -> str:
    if force or _stale(TESTING_LIB, ["-DPPCX_TESTING"]):
        _compile(TESTING_LIB, ["-DPPCX_TESTING"], verbose)
    return TESTING_LIB


def build_all(force: bool = False, verbose: bool = False):
    """The product and the testing build side by side (the sweep's translation units take minutes)."""
    jobs = []
    if force or _stale(LIB):
        jobs.append((LIB, []))
    if force or _stale(TESTING_LIB, ["-DPPCX_TESTING"]):
        jobs.append((TESTING_LIB, ["-DPPCX_TESTING"]))
    errs = []

    def run(lib, extra):
        try:
            _compile(lib, extra, verbose)
        except Exception as e:                   # noqa: BLE001 -- reported below
            errs.append(e)
    th = [threading.Thread(target=run, args=j) for j in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return LIB, TESTING_LIB


if __name__ == "__main__":
    if "--testing" in sys.argv:
        print(*build_all(force="--force" in sys.argv, verbose=True))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
