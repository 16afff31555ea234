"""The one recipe for the CPU builds of the kernel headers: tests/<name>_host/<name>_host.cpp (a name that ends in _twin:
tests/<name>/<name>.cpp) includes the header the gfx950 kernel includes and is compiled with g++, as a library that the tests
call through ctypes (host_lib) and, with -DPPCX_HOST_MAIN, as a stand-alone program with fixed inputs for a run under the host
sanitizers:

    python -m tests.host_build --sanitize [name ...]

builds each named program (all of NAMES without a name) with SANITIZE into a temporary directory and runs it as a child process
under a time limit, stopping with a non-zero status at the first that fails. That is a command for a CPU machine; nothing is
loaded into Python.

Whether a library is stale is the compiler's statement (g++ -MM), never a hand-written list of headers. The `emul` fixture of
tests/conftest.py builds tests/emul with the same flags and a list of its own; it is left as it is."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("psis", "summary", "reff", "loo", "loo_mcse", "loo_predict", "loo_ap", "ppc_exact", "loo_exact", "loo_mm", "loo_mm_exact",
         "loo_mm_split_twin", "loo_mm_cov_twin")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden"]
SANITIZE = ["-O1", "-g", "-std=c++17", "-DPPCX_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
RUN_SECONDS = 120                                     # a program's time limit under the sanitizers; each runs in well under 1 s


def program(name):
    """the program's, its directory's and its source's name"""
    return name if name.endswith("_twin") else name + "_host"


def source(name, root=ROOT):
    return os.path.join(root, "tests", program(name), program(name) + ".cpp")


def dependencies(src):
    """src and every file it includes, system headers aside, as g++ -MM lists them"""
    rule = subprocess.check_output(["g++", "-std=c++17", "-MM", src], text=True).replace("\\\n", " ")
    words = re.split(r"(?<!\\)\s+", rule.split(":", 1)[1].strip())
    return [os.path.normpath(w.replace("\\ ", " ")) for w in words]


def build(src, lib):
    """compile src into the library lib if lib is missing or older than one of src's dependencies; True if it compiled"""
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(p) for p in dependencies(src)):
        return False
    subprocess.check_call(["g++"] + FLAGS + ["-o", lib, src])
    return True


def host_lib(name, signatures, root=ROOT):
    """the ctypes.CDLL of source(name, root), built or reused; signatures: {function: (argtypes, restype)}"""
    src = source(name, root)
    lib = os.path.join(os.path.dirname(src), "lib" + program(name) + ".so")
    build(src, lib)
    h = ctypes.CDLL(lib)
    for fn, (argtypes, restype) in signatures.items():
        getattr(h, fn).argtypes, getattr(h, fn).restype = argtypes, restype
    return h


def sanitize(names):
    """build and run the stand-alone programs under the sanitizers; the exit status of the first that fails, or 0"""
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            exe = os.path.join(tmp, program(name))
            subprocess.check_call(["g++"] + SANITIZE + ["-o", exe, source(name)])
            print("---- " + program(name), flush=True)
            try:
                status = subprocess.run([exe], timeout=RUN_SECONDS).returncode
            except subprocess.TimeoutExpired:
                status = 124
            if status:
                print(f"{program(name)} failed under the sanitizers: exit status {status}", flush=True)
                return status
    print(f"{len(names)} programs clean under -fsanitize=address,undefined: " + " ".join(names))
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] != ["--sanitize"] or not set(args[1:]) <= set(NAMES):
        sys.exit("usage: python -m tests.host_build --sanitize [" + " | ".join(NAMES) + " ...]")
    sys.exit(sanitize(args[1:] or NAMES))
