"""ctypes binding of the C ABI in include/ppcx.h (libppcx.so, built by ppcseq_amd/build.py).

There is deliberately no CPU fallback: if the HIP library is missing or no MI355X is visible the
calls raise. The library is loaded from the package directory (in-tree build).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPCX_LIB", os.path.join(_HERE, "libppcx.so"))   # PPCX_LIB: development builds

EXPORTS = [
    "ppcx_version", "ppcx_device_count", "ppcx_last_error", "ppcx_model_create", "ppcx_model_set_exclusions",
    "ppcx_model_set_launch", "ppcx_model_get_launch", "ppcx_model_get_plan", "ppcx_model_dim", "ppcx_model_destroy", "ppcx_log_prob_grad",
    "ppcx_nuts_config_default", "ppcx_fit_nuts", "ppcx_fit_info", "ppcx_fit_from_draws", "ppcx_fit_get_draws", "ppcx_fit_get_columns",
    "ppcx_fit_get_diagnostics", "ppcx_fit_get_timing", "ppcx_fit_get_kernel_times", "ppcx_fit_ppc", "ppcx_fit_free", "ppcx_do_inference_C", "ppcx_model_set_rounds", "ppcx_model_get_rounds", "ppcx_model_set_progress",
    "ppcx_model_create_shard", "ppcx_model_create_shard_strided", "ppcx_fit_nuts_shards", "ppcx_comm_unique_id", "ppcx_comm_create", "ppcx_comm_destroy",
    "ppcx_fit_nuts_comm", "ppcx_advi_config_default", "ppcx_fit_advi", "ppcx_fit_advi_info", "ppcx_fit_advi_iterative",
    "ppcx_guard_decision", "ppcx_device_memory", "ppcx_fit_get_ppc_timing",
    "ppcx_xchg_create", "ppcx_xchg_handle", "ppcx_xchg_connect", "ppcx_xchg_connect_local", "ppcx_xchg_set_timeout", "ppcx_xchg_destroy",
    "ppcx_fit_nuts_xchg", "ppcx_fit_get_xchg_timing", "ppcx_fit_get_inv_metric", "ppcx_fit_summary",
    "ppcx_fit_get_approximation", "ppcx_fit_get_log_ratios", "ppcx_fit_psis", "ppcx_fit_get_log_lik", "ppcx_fit_loo",
    "ppcx_fit_loo_predict", "ppcx_fit_relative_eff", "ppcx_fit_loo_mcse", "ppcx_fit_loo_approx", "ppcx_fit_loo_predict_approx",
    "ppcx_fit_ppc_exact", "ppcx_fit_loo_predict_exact", "ppcx_fit_loo_predict_exact_approx", "ppcx_fit_loo_moment_match",
    "ppcx_fit_loo_predict_exact_moment_match", "ppcx_fit_loo_moment_match_split", "ppcx_fit_loo_predict_exact_moment_match_split",
    "ppcx_fit_loo_moment_match_cov", "ppcx_fit_loo_predict_exact_moment_match_cov",
    "ppcx_model_create_ex", "ppcx_model_get_per_sample",
    "ppcx_fit_loo_moment_match_approx", "ppcx_fit_loo_predict_exact_moment_match_approx",
]
PER_SAMPLE = {"lds": 0, "stream": 1, "auto": 2}     # PPCX_PER_SAMPLE_*
ABI_VERSION = 400           # include/ppcx.h PPCX_VERSION this binding was written for
SUMMARY_FIELDS = ("mean", "sd", "q05", "q50", "q95", "rhat", "ess_bulk", "ess_tail")   # PPCX_SUMMARY_FIELDS, in order
LOO_FIELDS = ("elpd_loo", "p_loo", "looic", "khat")                                      # PPCX_LOO_FIELDS, in order
LOO_MCSE_FIELDS = LOO_FIELDS + ("mcse_elpd_loo", "n_eff")                                # PPCX_LOO_MCSE_FIELDS, in order
LOO_PREDICT_FIELDS = ("mean", "lower", "upper", "pit_lt", "pit_le", "khat")              # PPCX_LOO_PREDICT_FIELDS, in order
PPC_EXACT_FIELDS = ("mean", "sd", "p_le", "p_ge", "lower", "upper", "y", "excluded", "outside")   # PPCX_PPC_EXACT_FIELDS, in order
LOO_EXACT_FIELDS = PPC_EXACT_FIELDS + ("khat",)                                          # PPCX_LOO_EXACT_FIELDS, in order
LOO_MM_HEAD = LOO_FIELDS + ("khat_before", "iterations")     # PPCX_LOO_MM_FIELDS(C): these, then scale[C + 1] and shift[C + 1]
LOO_MM_SPLIT_TAIL = ("elpd_loo_matched", "khat_split")       # PPCX_LOO_MM_SPLIT_FIELDS(C): PPCX_LOO_MM_FIELDS(C), then these
# PPCX_LOO_MM_COV_FIELDS(C): these, then transform[C + 1][C + 1] and shift[C + 1]
LOO_MM_COV_HEAD = LOO_MM_HEAD + ("cov_iterations",) + LOO_MM_SPLIT_TAIL


class PpcxError(RuntimeError):
    pass


class NutsConfig(C.Structure):
    _fields_ = [("chains", C.c_int), ("iter", C.c_int), ("warmup", C.c_int), ("seed", C.c_ulonglong),
                ("adapt_delta", C.c_double), ("max_treedepth", C.c_int), ("init_radius", C.c_double),
                ("stepsize0", C.c_double), ("init_buffer", C.c_int), ("term_buffer", C.c_int), ("window", C.c_int),
                ("chain_id_offset", C.c_int)]


class AdviConfig(C.Structure):
    _fields_ = [("output_samples", C.c_int), ("iter", C.c_int), ("tol_rel_obj", C.c_double), ("grad_samples", C.c_int),
                ("elbo_samples", C.c_int), ("eval_elbo", C.c_int), ("adapt_iter", C.c_int), ("seed", C.c_ulonglong),
                ("init_radius", C.c_double)]


PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_double)
_lib = None
_LACKING = ()


def use_library(path=None, lacking=()):
    """Bind another build of the library from now on (None: back to the product build). For the tests that need the
    testing build (tests/libppcx_testing.so: fault injection, forced cell paths, kernel-level timing); every Model / Fit /
    Comm of the previous library must have been closed. lacking: the entries of EXPORTS that the caller states the build at
    `path` does not have (an older build, scripts/gpu_cell_entries_time.py's parent); they are left unbound and calling one
    raises AttributeError. load() refuses a library that lacks any other entry."""
    global _lib, LIB_PATH, _LACKING
    _lib = None
    _LACKING = tuple(lacking) if path else ()
    LIB_PATH = path if path else os.environ.get("PPCX_LIB", os.path.join(_HERE, "libppcx.so"))


def load() -> C.CDLL:
    """Load libppcx.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PpcxError(f"{LIB_PATH} not found: run `python -m ppcseq_amd.build` (hipcc, gfx950) first; "
                        "there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    lib.ppcx_version.restype = C.c_int
    if lib.ppcx_version() != ABI_VERSION:
        raise PpcxError(f"{LIB_PATH} has ABI version {lib.ppcx_version()}, this binding needs {ABI_VERSION}: rebuild it "
                        "(`python -m ppcseq_amd.build --force`)")
    missing = [name for name in EXPORTS if name not in _LACKING and not hasattr(lib, name)]
    if missing:
        raise PpcxError(f"{LIB_PATH} lacks {', '.join(missing)}: rebuild it (`python -m ppcseq_amd.build --force`)")
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.ppcx_guard_decision.argtypes = [dp, C.c_int]
    lib.ppcx_device_memory.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.ppcx_fit_get_ppc_timing.argtypes = [C.c_void_p, dp, C.POINTER(C.c_longlong)]
    lib.ppcx_last_error.restype = C.c_char_p
    lib.ppcx_model_create.argtypes = [C.c_int] * 5 + [ip, dp, dp, C.c_double, C.c_int, ip, C.POINTER(C.c_void_p)]
    if "ppcx_model_create_ex" not in _LACKING:
        lib.ppcx_model_create_ex.argtypes = [C.c_int] * 5 + [ip, dp, dp, C.c_double, C.c_int, ip, C.c_int, C.POINTER(C.c_void_p)]
        lib.ppcx_model_get_per_sample.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.ppcx_model_set_exclusions.argtypes = [C.c_void_p, C.c_int, ip]
    lib.ppcx_model_set_launch.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.ppcx_model_get_launch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ppcx_model_get_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int]
    lib.ppcx_model_dim.argtypes = [C.c_void_p]
    lib.ppcx_model_destroy.argtypes = [C.c_void_p]
    lib.ppcx_model_destroy.restype = None
    lib.ppcx_log_prob_grad.argtypes = [C.c_void_p, C.c_int, dp, dp, dp]
    lib.ppcx_nuts_config_default.argtypes = [C.POINTER(NutsConfig)]
    lib.ppcx_nuts_config_default.restype = None
    lib.ppcx_fit_nuts.argtypes = [C.c_void_p, C.POINTER(NutsConfig), C.POINTER(C.c_void_p)]
    lib.ppcx_fit_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
    lib.ppcx_fit_from_draws.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, C.POINTER(C.c_void_p)]
    lib.ppcx_fit_get_draws.argtypes = [C.c_void_p, dp]
    lib.ppcx_fit_get_columns.argtypes = [C.c_void_p, C.c_int, ip, dp]
    lib.ppcx_fit_summary.argtypes = [C.c_void_p, C.c_int, ip, dp]
    lib.ppcx_fit_get_approximation.argtypes = [C.c_void_p, dp, dp]
    lib.ppcx_fit_get_log_ratios.argtypes = [C.c_void_p, dp, dp]
    lib.ppcx_fit_psis.argtypes = [C.c_void_p, C.c_int, ip, dp]
    lib.ppcx_fit_get_log_lik.argtypes = [C.c_void_p, C.c_int, ip, dp]
    lib.ppcx_fit_loo.argtypes = [C.c_void_p, C.c_int, ip, dp, dp]
    lib.ppcx_fit_loo_mcse.argtypes = [C.c_void_p, C.c_int, ip, dp, dp]
    lib.ppcx_fit_loo_moment_match.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double, C.c_int, dp]
    lib.ppcx_fit_loo_moment_match_split.argtypes = lib.ppcx_fit_loo_moment_match.argtypes
    lib.ppcx_fit_loo_moment_match_cov.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double, C.c_int, C.c_int, dp]
    lib.ppcx_fit_loo_predict.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double, C.c_double, C.c_double, C.c_ulonglong, dp]
    lib.ppcx_fit_relative_eff.argtypes = [C.c_void_p, C.c_int, ip, dp]
    lib.ppcx_fit_loo_approx.argtypes = [C.c_void_p, C.c_int, ip, dp]
    lib.ppcx_fit_loo_predict_approx.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, C.c_double, C.c_ulonglong, dp]
    lib.ppcx_fit_ppc_exact.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, C.c_double, dp]
    lib.ppcx_fit_loo_predict_exact.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double, C.c_double, C.c_double, dp]
    lib.ppcx_fit_loo_predict_exact_approx.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, C.c_double, dp]
    lib.ppcx_fit_loo_predict_exact_moment_match.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double, C.c_int, C.c_double, C.c_double,
                                                            C.c_double, dp]
    lib.ppcx_fit_loo_predict_exact_moment_match_split.argtypes = lib.ppcx_fit_loo_predict_exact_moment_match.argtypes
    if "ppcx_fit_loo_predict_exact_moment_match_cov" not in _LACKING:
        lib.ppcx_fit_loo_predict_exact_moment_match_cov.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_double, C.c_int, C.c_int, C.c_double,
                                                                    C.c_double, C.c_double, dp]
    if "ppcx_fit_loo_moment_match_approx" not in _LACKING:
        lib.ppcx_fit_loo_moment_match_approx.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_int, dp]
        lib.ppcx_fit_loo_predict_exact_moment_match_approx.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_int, C.c_double,
                                                                       C.c_double, C.c_double, dp]
    lib.ppcx_fit_get_diagnostics.argtypes = [C.c_void_p, dp, dp, ip, ip, ip, dp]
    lib.ppcx_fit_get_timing.argtypes = [C.c_void_p, dp, C.POINTER(C.c_longlong), dp, C.POINTER(C.c_longlong), dp]
    lib.ppcx_fit_get_kernel_times.argtypes = [C.c_void_p, dp, dp, dp, C.POINTER(C.c_longlong)]
    lib.ppcx_fit_get_inv_metric.argtypes = [C.c_void_p, dp]
    lib.ppcx_fit_ppc.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_ulonglong, C.c_int, C.c_int, dp, ip]
    lib.ppcx_fit_free.argtypes = [C.c_void_p]
    lib.ppcx_model_set_rounds.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.ppcx_xchg_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ppcx_xchg_handle.argtypes = [C.c_void_p, C.c_char_p]
    lib.ppcx_xchg_connect.argtypes = [C.c_void_p, C.c_char_p]
    lib.ppcx_xchg_connect_local.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.ppcx_xchg_set_timeout.argtypes = [C.c_void_p, C.c_double]
    lib.ppcx_xchg_destroy.argtypes = [C.c_void_p]
    lib.ppcx_xchg_destroy.restype = None
    lib.ppcx_fit_nuts_xchg.argtypes = [C.c_void_p, C.POINTER(NutsConfig), C.c_void_p, C.POINTER(C.c_void_p)]
    lib.ppcx_fit_get_xchg_timing.argtypes = [C.c_void_p, dp, C.POINTER(C.c_longlong)]
    lib.ppcx_model_get_rounds.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ppcx_model_set_progress.argtypes = [C.c_void_p, PROGRESS_FN, C.c_void_p, C.c_double]
    if hasattr(lib, "ppcx_testing_set"):         # the testing build (csrc/ppcx_testing.h)
        lib.ppcx_testing_set.argtypes = [C.c_char_p, C.c_longlong]
        lib.ppcx_testing_set_nccl_provider.argtypes = [C.c_char_p]
        lib.ppcx_testing_bench_kernel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.POINTER(C.c_int)]
    # the element-wise math and table read-back hooks: bound only where the testing build has them, so that a testing build of
    # an older source still loads (its hooks above keep working; testing_eval_math / testing_disp_table then raise)
    if hasattr(lib, "ppcx_testing_eval_math"):
        lib.ppcx_testing_eval_math.argtypes = [C.c_int, C.c_int, dp, dp, ip, dp, dp]
    if hasattr(lib, "ppcx_testing_get_disp_table"):
        lib.ppcx_testing_get_disp_table.argtypes = [C.c_void_p, dp]
    if hasattr(lib, "ppcx_testing_psis"):
        lib.ppcx_testing_psis.argtypes = [C.c_int, C.c_int, dp, dp, dp]
    if hasattr(lib, "ppcx_testing_loo"):
        lib.ppcx_testing_loo.argtypes = [C.c_int, C.c_int, dp, ip, dp, dp]
    if hasattr(lib, "ppcx_testing_loo_mcse"):
        lib.ppcx_testing_loo_mcse.argtypes = [C.c_int, C.c_int, dp, ip, dp, dp]
    if hasattr(lib, "ppcx_testing_loo_predict"):
        lib.ppcx_testing_loo_predict.argtypes = [dp, ip, C.c_int, C.c_int, ip, ip, dp, C.c_double, C.c_double, dp]
    if hasattr(lib, "ppcx_testing_loo_approx"):
        lib.ppcx_testing_loo_approx.argtypes = [C.c_int, C.c_int, dp, dp, ip, dp]
        lib.ppcx_testing_loo_predict_approx.argtypes = [dp, dp, ip, C.c_int, C.c_int, ip, ip, C.c_double, C.c_double, dp]
    if hasattr(lib, "ppcx_testing_relative_eff"):
        lib.ppcx_testing_relative_eff.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp]
    if hasattr(lib, "ppcx_testing_ppc_exact"):
        lib.ppcx_testing_ppc_exact.argtypes = [C.c_int, C.c_int, dp, dp, ip, ip, C.c_double, C.c_double, C.c_double, dp]
    if hasattr(lib, "ppcx_testing_loo_exact"):
        lib.ppcx_testing_loo_exact.argtypes = [C.c_int, C.c_int, dp, dp, dp, ip, ip, dp, dp, C.c_double, C.c_double, C.c_double, dp]
    if hasattr(lib, "ppcx_testing_fit_from_draws_approx"):
        lib.ppcx_testing_fit_from_draws_approx.argtypes = [C.c_void_p, C.c_int, dp, dp, C.POINTER(C.c_void_p)]
    lib.ppcx_fit_free.restype = None
    lib.ppcx_advi_config_default.argtypes = [C.POINTER(AdviConfig)]
    lib.ppcx_advi_config_default.restype = None
    lib.ppcx_fit_advi.argtypes = [C.c_void_p, C.POINTER(AdviConfig), C.POINTER(C.c_void_p)]
    lib.ppcx_fit_advi_iterative.argtypes = [C.c_void_p, C.POINTER(AdviConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.ppcx_fit_advi_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ppcx_model_create_shard.argtypes = [C.c_int] * 7 + [ip, dp, dp, C.c_double, C.c_int, ip, C.POINTER(C.c_void_p)]
    lib.ppcx_model_create_shard_strided.argtypes = [C.c_int] * 8 + [ip, dp, dp, C.c_double, C.c_int, ip, C.POINTER(C.c_void_p)]
    lib.ppcx_fit_nuts_shards.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(NutsConfig), C.POINTER(C.c_void_p)]
    lib.ppcx_comm_unique_id.argtypes = [C.c_char_p]
    lib.ppcx_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.ppcx_comm_destroy.argtypes = [C.c_void_p]
    lib.ppcx_comm_destroy.restype = None
    lib.ppcx_fit_nuts_comm.argtypes = [C.c_void_p, C.POINTER(NutsConfig), C.c_void_p, C.POINTER(C.c_void_p)]
    _lib = lib
    return lib


def _check(rc: int):
    if rc != 0:
        raise PpcxError(f"ppcx error {rc}: {load().ppcx_last_error().decode()}")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _testing_entry(name):
    """The entry `name` of the testing build (csrc/ppcx_testing.h); the product build has none."""
    lib = load()
    if not hasattr(lib, name):
        raise PpcxError(f"{LIB_PATH} is not the testing build, or one built before {name} existed: rebuild it "
                        "(`python -m ppcseq_amd.build --testing --force`)")
    return getattr(lib, name)


def testing_set(key: str, value: int):
    """A test hook of the testing build (csrc/ppcx_testing.h); the product build has none."""
    fn = _testing_entry("ppcx_testing_set")
    _check(fn(key.encode(), int(value)))


def testing_set_nccl_provider(path: str):
    fn = _testing_entry("ppcx_testing_set_nccl_provider")
    _check(fn(path.encode() if path else None))


# function ids of ppcx_testing_eval_math (csrc/ppcx_testing.h PPCX_MATH_*)
TESTING_MATH = ("fast_rcp", "fast_log", "fast_exp", "table_log", "window_log", "stirling_tails", "stirling_excess",
                "log_erfc_ratio", "cell", "cell_win", "cell_y", "cell_win_y", "sincos_2pi", "lgamma_int1", "rng_exp", "rng_div")
# ... and those of the headers beside ppcx_math.h / ppcx_model.h, whose ids go on from there (ppcx_nbcdf.h: PPCX_MATH_NB2_TAILS);
# the CPU emulation harness knows the ids of TESTING_MATH only
TESTING_MATH_MORE = ("nb2_tails",)


def testing_eval_math(fn: str, a, b=None, y=None):
    """(out0, out1) of one of the device's building blocks at every element of a, b, y (testing build only;
    csrc/ppcx_testing.h ppcx_testing_eval_math)."""
    entry = _testing_entry("ppcx_testing_eval_math")
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    n = a.size
    b = np.ascontiguousarray(np.zeros(n) if b is None else np.broadcast_to(b, (n,)), dtype=np.float64)
    y = np.ascontiguousarray(np.zeros(n) if y is None else np.broadcast_to(y, (n,)), dtype=np.int32)
    o0, o1 = np.zeros(n), np.zeros(n)
    rc = entry((TESTING_MATH + TESTING_MATH_MORE).index(fn), n, _p(a, C.c_double), _p(b, C.c_double), _p(y, C.c_int32),
               _p(o0, C.c_double), _p(o1, C.c_double))
    if rc != 0:
        raise PpcxError(f"ppcx_testing_eval_math({fn}) failed with code {rc}")
    return o0, o1


def testing_psis(lr, cols=None):
    """k-hat of the PSIS kernel on host-given values (testing build only; csrc/ppcx_testing.h ppcx_testing_psis): lr [n] log
    ratios, cols [n, n_cols] parameter draws or None. Returns [n_cols + 1]: the columns' k-hat, then that of lr itself."""
    fn = _testing_entry("ppcx_testing_psis")
    lr = np.ascontiguousarray(lr, dtype=np.float64).ravel()
    n = lr.size
    cols = np.zeros((n, 0)) if cols is None else np.ascontiguousarray(cols, dtype=np.float64).reshape(n, -1)
    out = np.zeros(cols.shape[1] + 1)
    _check(fn(n, int(cols.shape[1]), _p(lr, C.c_double), _p(cols, C.c_double) if cols.size else None, _p(out, C.c_double)))
    return out


def testing_loo(ll, excluded=None, r_eff=None):
    """PSIS-LOO kernel on host-given log-likelihood columns (testing build only; csrc/ppcx_testing.h ppcx_testing_loo): ll
    [n_draws, n_cells], excluded / r_eff None or [n_cells]. Returns [n_cells, 4]: elpd_loo, p_loo, looic, khat."""
    return _testing_loo("ppcx_testing_loo", LOO_FIELDS, ll, excluded, r_eff)


def testing_loo_mcse(ll, excluded=None, r_eff=None):
    """testing_loo as ppcx_fit_loo_mcse runs the kernel (csrc/ppcx_testing.h ppcx_testing_loo_mcse). Returns [n_cells, 6]:
    elpd_loo, p_loo, looic, khat, mcse_elpd_loo, n_eff."""
    return _testing_loo("ppcx_testing_loo_mcse", LOO_MCSE_FIELDS, ll, excluded, r_eff)


def _testing_loo(entry, fields, ll, excluded, r_eff):
    fn = _testing_entry(entry)
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(ll.shape[0], -1)
    n, nc = ll.shape
    cols = np.ascontiguousarray(ll.T)
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32).ravel()
    re = None if r_eff is None else np.ascontiguousarray(r_eff, dtype=np.float64).ravel()
    out = np.zeros((nc, len(fields)))
    _check(fn(n, nc, _p(cols, C.c_double), _p(ex, C.c_int32), _p(re, C.c_double), _p(out, C.c_double)))
    return out


def testing_loo_predict(ll, x, y, excluded=None, r_eff=None, p_lo=0.025, p_hi=0.975):
    """The kernel of ppcx_fit_loo_predict on host-given columns (testing build only; csrc/ppcx_testing.h
    ppcx_testing_loo_predict): ll [n_draws, n_cells] log-likelihoods, x [n_draws, n_cells] predictive counts, y [n_cells] observed
    counts, excluded / r_eff None or [n_cells]. Returns [n_cells, 6]: mean, lower, upper, pit_lt, pit_le, khat."""
    fn = _testing_entry("ppcx_testing_loo_predict")
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(ll.shape[0], -1)
    n, nc = ll.shape
    cols = np.ascontiguousarray(ll.T)
    xs = np.ascontiguousarray(np.asarray(x).reshape(n, nc).T, dtype=np.int32)
    ys = np.ascontiguousarray(np.broadcast_to(np.asarray(y), (nc,)), dtype=np.int32)
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32).ravel()
    re = None if r_eff is None else np.ascontiguousarray(r_eff, dtype=np.float64).ravel()
    out = np.zeros((nc, len(LOO_PREDICT_FIELDS)))
    _check(fn(_p(cols, C.c_double), _p(xs, C.c_int32), n, nc, _p(ys, C.c_int32), _p(ex, C.c_int32), _p(re, C.c_double),
              float(p_lo), float(p_hi), _p(out, C.c_double)))
    return out


def _testing_approx_columns(entry, ll, log_ratio, excluded):
    """What the two approximate-posterior test entries share: the library, ll as [n_cells][n], log_ratio [n], the flags"""
    fn = _testing_entry(entry)
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(ll.shape[0], -1)
    lr = np.ascontiguousarray(log_ratio, dtype=np.float64).ravel()
    if lr.size != ll.shape[0]:
        raise ValueError("log_ratio must hold one value per draw")
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32).ravel()
    return fn, np.ascontiguousarray(ll.T), lr, ex


def testing_loo_approx(ll, log_ratio, excluded=None):
    """The kernel of ppcx_fit_loo_approx on host-given columns (testing build only; csrc/ppcx_testing.h ppcx_testing_loo_approx):
    ll [n_draws, n_cells], log_ratio [n_draws] (log_p - log_g of the draws), excluded None or [n_cells]. Returns [n_cells, 4]:
    elpd_loo, p_loo, looic, khat."""
    fn, cols, lr, ex = _testing_approx_columns("ppcx_testing_loo_approx", ll, log_ratio, excluded)
    nc, n = cols.shape
    out = np.zeros((nc, len(LOO_FIELDS)))
    _check(fn(n, nc, _p(cols, C.c_double), _p(lr, C.c_double), _p(ex, C.c_int32), _p(out, C.c_double)))
    return out


def testing_loo_predict_approx(ll, log_ratio, x, y, excluded=None, p_lo=0.025, p_hi=0.975):
    """The kernel of ppcx_fit_loo_predict_approx on host-given columns (testing build only; csrc/ppcx_testing.h
    ppcx_testing_loo_predict_approx): as testing_loo_predict with log_ratio [n_draws] and r_eff = 1. Returns [n_cells, 6]."""
    fn, cols, lr, ex = _testing_approx_columns("ppcx_testing_loo_predict_approx", ll, log_ratio, excluded)
    nc, n = cols.shape
    xs = np.ascontiguousarray(np.asarray(x).reshape(n, nc).T, dtype=np.int32)
    ys = np.ascontiguousarray(np.broadcast_to(np.asarray(y), (nc,)), dtype=np.int32)
    out = np.zeros((nc, len(LOO_PREDICT_FIELDS)))
    _check(fn(_p(cols, C.c_double), _p(lr, C.c_double), _p(xs, C.c_int32), n, nc, _p(ys, C.c_int32), _p(ex, C.c_int32),
              float(p_lo), float(p_hi), _p(out, C.c_double)))
    return out


def testing_relative_eff(ll, chains):
    """The kernel of ppcx_fit_relative_eff on host-given log-likelihood columns (testing build only; csrc/ppcx_testing.h
    ppcx_testing_relative_eff): ll [chains * n, n_cells], the draws chain-major. Returns [n_cells]."""
    fn = _testing_entry("ppcx_testing_relative_eff")
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(ll.shape[0], -1)
    rows, nc = ll.shape
    chains = int(chains)
    if chains < 1 or rows % chains:
        raise ValueError("ll must hold chains * n rows")
    cols = np.ascontiguousarray(ll.T)
    out = np.zeros(nc)
    _check(fn(chains, rows // chains, nc, _p(cols, C.c_double), _p(out, C.c_double)))
    return out


def _ppc_exact_dict(out):
    """[.., PPC_EXACT_FIELDS] as the dict of Fit.ppc_exact: y and the interval ends integers (-1 where the cell is NaN), excluded
    and outside booleans (outside False where the cell is NaN)"""
    res = {k: out[..., i].copy() for i, k in enumerate(PPC_EXACT_FIELDS)}
    nan = np.isnan(res["lower"]) | np.isnan(res["upper"])
    for k in ("lower", "upper"):
        res[k] = np.where(nan, -1, res[k]).astype(np.int64)
    res["y"] = res["y"].astype(np.int64)
    res["excluded"] = res["excluded"] != 0
    res["outside"] = np.where(nan, 0, res["outside"]) != 0
    return res


def testing_ppc_exact(eta, sigma_raw, y, excluded=None, truncation_compensation=1.0, p_lo=0.025, p_hi=0.975, raw=False):
    """The kernel of ppcx_fit_ppc_exact on host-given columns (testing build only; csrc/ppcx_testing.h ppcx_testing_ppc_exact):
    eta, sigma_raw [n_draws, n_cells], y [n_cells] observed counts, excluded None or [n_cells]. Returns Fit.ppc_exact's dict of
    [n_cells] arrays, or with raw=True the [n_cells, 9] doubles as the kernel wrote them."""
    fn = _testing_entry("ppcx_testing_ppc_exact")
    eta = np.asarray(eta, dtype=np.float64)
    eta = eta.reshape(eta.shape[0], -1)
    n, nc = eta.shape
    ec = np.ascontiguousarray(eta.T)
    sc = np.ascontiguousarray(np.asarray(sigma_raw, dtype=np.float64).reshape(n, nc).T)
    ys = np.ascontiguousarray(np.broadcast_to(np.asarray(y), (nc,)), dtype=np.int32)
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32).ravel()
    out = np.zeros((nc, len(PPC_EXACT_FIELDS)))
    _check(fn(n, nc, _p(ec, C.c_double), _p(sc, C.c_double), _p(ys, C.c_int32), _p(ex, C.c_int32), float(truncation_compensation),
              float(p_lo), float(p_hi), _p(out, C.c_double)))
    return out if raw else _ppc_exact_dict(out)


def _loo_exact_dict(out):
    """[.., LOO_EXACT_FIELDS] as the dict of Fit.loo_predict_exact: _ppc_exact_dict's keys and dtypes, khat, and the two ends of
    the randomised LOO-PIT under Fit.loo_predict's names: pit_lt = 1 - p_ge, pit_le = p_le"""
    res = _ppc_exact_dict(out)
    res["khat"] = out[..., len(PPC_EXACT_FIELDS)].copy()
    res["pit_lt"] = 1.0 - res["p_ge"]
    res["pit_le"] = res["p_le"].copy()
    return res


def testing_loo_exact(ll, eta, sigma_raw, y, excluded=None, r_eff=None, log_ratio=None, truncation_compensation=1.0, p_lo=0.025,
                      p_hi=0.975, raw=False):
    """The kernel of ppcx_fit_loo_predict_exact on host-given columns (testing build only; csrc/ppcx_testing.h
    ppcx_testing_loo_exact): ll, eta, sigma_raw [n_draws, n_cells], y [n_cells] observed counts, excluded / r_eff None or
    [n_cells]; log_ratio None, or [n_draws] (log_p - log_g of the draws): the kernel as ppcx_fit_loo_predict_exact_approx runs it.
    Returns Fit.loo_predict_exact's dict of [n_cells] arrays, or with raw=True the [n_cells, 10] doubles as the kernel wrote them."""
    fn = _testing_entry("ppcx_testing_loo_exact")
    ll = np.asarray(ll, dtype=np.float64)
    ll = ll.reshape(ll.shape[0], -1)
    n, nc = ll.shape
    lc = np.ascontiguousarray(ll.T)
    ec = np.ascontiguousarray(np.asarray(eta, dtype=np.float64).reshape(n, nc).T)
    sc = np.ascontiguousarray(np.asarray(sigma_raw, dtype=np.float64).reshape(n, nc).T)
    ys = np.ascontiguousarray(np.broadcast_to(np.asarray(y), (nc,)), dtype=np.int32)
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32).ravel()
    re = None if r_eff is None else np.ascontiguousarray(np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (nc,)))
    lr = None if log_ratio is None else np.ascontiguousarray(log_ratio, dtype=np.float64).ravel()
    if lr is not None and lr.size != n:
        raise ValueError("log_ratio must hold one value per draw")
    out = np.zeros((nc, len(LOO_EXACT_FIELDS)))
    _check(fn(n, nc, _p(lc, C.c_double), _p(ec, C.c_double), _p(sc, C.c_double), _p(ys, C.c_int32), _p(ex, C.c_int32),
              _p(re, C.c_double), _p(lr, C.c_double), float(truncation_compensation), float(p_lo), float(p_hi), _p(out, C.c_double)))
    return out if raw else _loo_exact_dict(out)


def loo_estimates(pointwise, excluded):
    """loo's `estimates` for elpd_loo, p_loo and looic over the non-excluded cells: {name: (sum, sqrt(n var))}, var of ddof 1"""
    keep = ~np.asarray(excluded, bool)
    out = {}
    for name in LOO_FIELDS[:3]:
        v = np.asarray(pointwise[name], dtype=np.float64)[keep]
        se = float(np.sqrt(v.size * np.var(v, ddof=1))) if v.size > 1 else float("nan")
        out[name] = (float(np.sum(v)), se)
    return out


def device_count() -> int:
    return int(load().ppcx_device_count())


def device_memory(device=0):
    """(free, total) bytes of a HIP device."""
    f, t = C.c_ulonglong(), C.c_ulonglong()
    _check(load().ppcx_device_memory(int(device), C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def shard_genes(G_total, g0, stride):
    """The genes of a strided shard (ppcx_model_create_shard_strided): g0, g0 + stride, ... below G_total."""
    return list(range(int(g0), int(G_total), int(stride)))


class Model:
    """Device-resident model inputs (Stan data block in logical form, include/ppcx.h)."""

    def __init__(self, counts, X, exposure_rate, K, lambda_mu_mu=5.612671, excl=None, device=0, shard=None, per_sample="lds"):
        """per_sample: where the log-likelihood kernel keeps the per-sample constants (include/ppcx.h ppcx_model_create_ex) --
        "lds" (S * C doubles must fit LDS beside the tables: PpcxError beyond), "stream" (read from global memory), "auto" (LDS
        where it fits, streamed beyond); Model.per_sample says which of the two the model runs. Gene shards stay on "lds".
        shard = (G_total, K_total, g0, g1): `counts` then holds only genes [g0, g1) of the whole problem and K is
        ignored (the shard's checked genes are those of the first K_total that fall in its range). shard = (G_total, K_total,
        g0, None, stride): the genes g0, g0 + stride, ... of the whole problem -- rank r of N with (r, None, N) is the
        reference's round-robin deal of genes to shards (R/utilities.R:125-136; shard_genes() picks the rows)."""
        if per_sample not in PER_SAMPLE:
            raise ValueError('per_sample must be "lds", "stream" or "auto"')
        if shard is not None and per_sample != "lds":
            raise ValueError('a gene shard keeps the per-sample constants in LDS: per_sample must be "lds" with shard=')
        lib = load()
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if counts.ndim != 2:
            raise ValueError("counts must be G x S")
        self.G, self.S = counts.shape
        X = np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(self.S, -1))
        self.C = X.shape[1]
        self.K = int(K)
        exposure_rate = np.ascontiguousarray(exposure_rate, dtype=np.float64)
        if exposure_rate.shape != (self.S,):
            raise ValueError("exposure_rate must have length S")
        excl = np.ascontiguousarray(excl if excl is not None else np.zeros(0), dtype=np.int32)
        self.X, self.exposure_rate = X, exposure_rate
        self.excl = excl.copy()                  # the cells excluded now (Fit.loo holds them out)
        self.counts = counts                     # the observed counts (Fit.loo_predict reports them beside the intervals)
        h = C.c_void_p()
        self.shard = shard
        if shard is None and per_sample != "lds":
            _check(lib.ppcx_model_create_ex(int(device), self.G, self.S, self.C, self.K, _p(counts, C.c_int32),
                                            _p(X, C.c_double), _p(exposure_rate, C.c_double), float(lambda_mu_mu),
                                            int(excl.size), _p(excl, C.c_int32), PER_SAMPLE[per_sample], C.byref(h)))
        elif shard is None:
            _check(lib.ppcx_model_create(int(device), self.G, self.S, self.C, self.K, _p(counts, C.c_int32),
                                         _p(X, C.c_double), _p(exposure_rate, C.c_double), float(lambda_mu_mu),
                                         int(excl.size), _p(excl, C.c_int32), C.byref(h)))
        else:
            if len(shard) == 5:
                Gt, Kt, g0, stride = int(shard[0]), int(shard[1]), int(shard[2]), int(shard[4])
                if len(shard_genes(Gt, g0, stride)) != self.G:
                    raise ValueError("counts must hold exactly the genes of the shard")
                self.K = len([g for g in shard_genes(Gt, g0, stride) if g < Kt])
                _check(lib.ppcx_model_create_shard_strided(int(device), Gt, self.S, self.C, Kt, g0, stride, self.G, _p(counts, C.c_int32),
                                                           _p(X, C.c_double), _p(exposure_rate, C.c_double), float(lambda_mu_mu),
                                                           int(excl.size), _p(excl, C.c_int32), C.byref(h)))
            else:
                Gt, Kt, g0, g1 = (int(v) for v in shard)
                if g1 - g0 != self.G:
                    raise ValueError("counts must hold exactly the genes of the shard")
                self.K = max(0, min(g1, Kt) - min(g0, Kt))
                _check(lib.ppcx_model_create_shard(int(device), Gt, self.S, self.C, Kt, g0, g1, _p(counts, C.c_int32),
                                                   _p(X, C.c_double), _p(exposure_rate, C.c_double), float(lambda_mu_mu),
                                                   int(excl.size), _p(excl, C.c_int32), C.byref(h)))
        self._h = h
        self.D = int(lib.ppcx_model_dim(h))

    @property
    def per_sample(self):
        """"lds" or "stream": where this model's log-likelihood kernel reads the per-sample constants."""
        v = C.c_int()
        _check(load().ppcx_model_get_per_sample(self._h, C.byref(v)))
        return "stream" if v.value else "lds"

    def set_exclusions(self, excl):
        excl = np.ascontiguousarray(excl if excl is not None else np.zeros(0), dtype=np.int32)
        _check(load().ppcx_model_set_exclusions(self._h, int(excl.size), _p(excl, C.c_int32)))
        self.excl = excl.copy()

    def set_launch(self, lanes_per_gene=0, workgroups=0):
        """Pin the log-likelihood kernel's lanes per gene (a power of two <= 64) and/or its number of persistent
        workgroups; 0 = automatic. Results depend on lanes_per_gene only (summation order inside a gene)."""
        _check(load().ppcx_model_set_launch(self._h, int(lanes_per_gene), int(workgroups)))

    def get_plan(self, nchains):
        """(lanes per gene, workgroups per chain, bounds) of the log-likelihood launch planned for `nchains` chains:
        wavefront j of a chain walks the gene-order positions bounds[j] .. bounds[j + 1] - 1 (diagnostic). nchains < 0:
        the launch of -nchains chains of one of several chain groups, at the lanes per gene in force."""
        lanes, nb = C.c_int(), C.c_int()
        _check(load().ppcx_model_get_plan(self._h, int(nchains), C.byref(lanes), C.byref(nb), None, 0))
        b = np.zeros(4 * nb.value + 1, np.int32)
        _check(load().ppcx_model_get_plan(self._h, int(nchains), C.byref(lanes), C.byref(nb), _p(b, C.c_int32), int(b.size)))
        return lanes.value, nb.value, b

    def get_launch(self):
        a, b = C.c_int(), C.c_int()
        _check(load().ppcx_model_get_launch(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def testing_disp_table(self):
        """The dispersion tables the device built, [G][panel][function][12] (ppcx_disp.h layout; testing build only)."""
        fn = _testing_entry("ppcx_testing_get_disp_table")
        out = np.zeros((self.G, 32, 2, 12))
        _check(fn(self._h, _p(out, C.c_double)))
        return out

    def log_prob_grad(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        one = u.ndim == 1
        u2 = u.reshape(-1, self.D)
        lp = np.zeros(u2.shape[0])
        g = np.zeros_like(u2)
        _check(load().ppcx_log_prob_grad(self._h, u2.shape[0], _p(u2, C.c_double), _p(lp, C.c_double), _p(g, C.c_double)))
        return (float(lp[0]), g[0]) if one else (lp, g)

    def fit_nuts(self, chains=3, iter=300, warmup=150, seed=1, adapt_delta=0.8, max_treedepth=10, init_radius=2.0,
                 stepsize0=1.0, init_buffer=75, term_buffer=50, window=25, chain_id_offset=0) -> "Fit":
        cfg = NutsConfig(chains, iter, warmup, seed, adapt_delta, max_treedepth, init_radius, stepsize0,
                         init_buffer, term_buffer, window, chain_id_offset)
        h = C.c_void_p()
        _check(load().ppcx_fit_nuts(self._h, C.byref(cfg), C.byref(h)))
        return Fit(self, h)

    def fit_advi(self, output_samples=1000, iter=50000, tol_rel_obj=0.005, elbo_samples=100, eval_elbo=100, adapt_iter=50,
                 seed=1, init_radius=2.0, max_attempts=1) -> "Fit":
        """Mean-field ADVI (rstan::vb); returns a one-chain Fit holding output_samples draws of the approximation.
        max_attempts > 1: the bounded vb_iterative retry (R/utilities.R:246-278), attempt k with seed + k."""
        cfg = AdviConfig(output_samples, iter, tol_rel_obj, 1, elbo_samples, eval_elbo, adapt_iter, seed, init_radius)
        h = C.c_void_p()
        if max_attempts > 1:
            _check(load().ppcx_fit_advi_iterative(self._h, C.byref(cfg), int(max_attempts), C.byref(h)))
        else:
            _check(load().ppcx_fit_advi(self._h, C.byref(cfg), C.byref(h)))
        return Fit(self, h)

    def fit_from_draws(self, draws) -> "Fit":
        """A Fit over draws produced elsewhere ([chains, n_keep, D], unconstrained): pooled chains of other ranks."""
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim != 3 or draws.shape[2] != self.D:
            raise ValueError("draws must be [chains, n_keep, D]")
        h = C.c_void_p()
        _check(load().ppcx_fit_from_draws(self._h, draws.shape[0], draws.shape[1], _p(draws, C.c_double), C.byref(h)))
        return Fit(self, h)

    def testing_fit_from_draws_approx(self, draws, log_ratio) -> "Fit":
        """Testing build only (csrc/ppcx_testing.h ppcx_testing_fit_from_draws_approx): a Fit over host-given draws [n_keep, D] and
        host-given log ratios log_p - log_g [n_keep] that the approximate-posterior methods accept."""
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        log_ratio = np.ascontiguousarray(log_ratio, dtype=np.float64)
        if draws.ndim != 2 or draws.shape[1] != self.D or log_ratio.shape != (draws.shape[0],):
            raise ValueError("draws must be [n_keep, D] and log_ratio [n_keep]")
        h = C.c_void_p()
        _check(_testing_entry("ppcx_testing_fit_from_draws_approx")(self._h, draws.shape[0], _p(draws, C.c_double),
                                                                     _p(log_ratio, C.c_double), C.byref(h)))
        return Fit(self, h)

    def fit_nuts_comm(self, comm: "Comm", **kw) -> "Fit":
        """This process's gene shard of a multi-GPU fit; partial sums all-reduced over RCCL every leapfrog."""
        cfg = _make_cfg(**kw)
        h = C.c_void_p()
        _check(load().ppcx_fit_nuts_comm(self._h, C.byref(cfg), comm._h, C.byref(h)))
        return Fit(self, h)

    def fit_nuts_xchg(self, xchg: "Xchg", **kw) -> "Fit":
        """This rank's gene shard of a multi-GPU fit; the ranks' partial sums are exchanged directly by the state machines."""
        cfg = _make_cfg(**kw)
        h = C.c_void_p()
        _check(load().ppcx_fit_nuts_xchg(self._h, C.byref(cfg), xchg._h, C.byref(h)))
        return Fit(self, h)

    def set_rounds(self, pipelined=-2, stream_groups=-1):
        """Round structure of this model's NUTS fits: pipelined -1 = wherever the model allows it (the library's default), 0 = the
        three-launch round; stream_groups 0 = by the number of chains (the library's default), n = n chain groups on their own
        streams. An argument left out (-2 / -1) leaves that setting as it is."""
        _check(load().ppcx_model_set_rounds(self._h, int(pipelined), int(stream_groups)))

    def set_progress(self, fn=None, every_seconds=1.0):
        """fn(first_chain, chains, chains_done, rounds, seconds) during a NUTS fit of this model (None: off). A true return
        value ends the fit: the fit call raises PpcxError (PPCX_ERR_CANCELLED, -7), the model stays usable."""
        self._progress_cb = PROGRESS_FN((lambda user, c0, n, done, rounds, sec: 1 if fn(c0, n, done, rounds, sec) else 0) if fn else 0)
        _check(load().ppcx_model_set_progress(self._h, self._progress_cb, None, float(every_seconds)))

    def get_rounds(self, nchains=1):
        """(pipelined, stream_groups) a fit of `nchains` chains would run with."""
        a, b = C.c_int(), C.c_int()
        _check(load().ppcx_model_get_rounds(self._h, int(nchains), C.byref(a), C.byref(b)))
        return bool(a.value), b.value

    def bench_kernel(self, which=0, nchains=1, warm_rounds=40, reps=50, n_merge=1):
        """(ms per launch, command type) of one kernel of the three-launch round -- testing build only."""
        fn = _testing_entry("ppcx_testing_bench_kernel")
        ms, t = C.c_double(), C.c_int()
        _check(fn(self._h, int(which), nchains, warm_rounds, reps, n_merge, C.byref(ms), C.byref(t)))
        return ms.value, t.value

    def close(self):
        if getattr(self, "_h", None):
            load().ppcx_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _make_cfg(chains=3, iter=300, warmup=150, seed=1, adapt_delta=0.8, max_treedepth=10, init_radius=2.0,
              stepsize0=1.0, init_buffer=75, term_buffer=50, window=25, chain_id_offset=0):
    return NutsConfig(chains, iter, warmup, seed, adapt_delta, max_treedepth, init_radius, stepsize0,
                      init_buffer, term_buffer, window, chain_id_offset)


def fit_nuts_shards(models, **kw):
    """Gene-sharded fit with every shard in this process (one device): returns one Fit per shard."""
    cfg = _make_cfg(**kw)
    n = len(models)
    hm = (C.c_void_p * n)(*[m._h for m in models])
    hf = (C.c_void_p * n)()
    _check(load().ppcx_fit_nuts_shards(hm, n, C.byref(cfg), hf))
    return [Fit(m, C.c_void_p(h)) for m, h in zip(models, hf)]


class Comm:
    """RCCL communicator of a gene-sharded multi-GPU fit (one rank per GPU)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(load().ppcx_comm_unique_id(buf))
        return buf.raw

    def __init__(self, nranks, rank, unique_id: bytes, device=0):
        h = C.c_void_p()
        _check(load().ppcx_comm_create(int(device), int(nranks), int(rank), unique_id, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            load().ppcx_comm_destroy(self._h)
            self._h = None


class Xchg:
    """Direct-exchange group of a gene-sharded fit (include/ppcx.h ppcx_xchg_*): one rank per process and GPU, connected
    through IPC handles that the host layer all-gathers; or all ranks in this process (Xchg.local_group)."""

    def __init__(self, nranks, rank, max_chains, device=0):
        h = C.c_void_p()
        _check(load().ppcx_xchg_create(int(device), int(nranks), int(rank), int(max_chains), C.byref(h)))
        self._h, self.nranks, self.rank = h, int(nranks), int(rank)

    def handle(self) -> bytes:
        buf = C.create_string_buffer(64)
        _check(load().ppcx_xchg_handle(self._h, buf))
        return buf.raw

    def connect(self, handles):
        """handles: the ranks' 64-byte handles in rank order."""
        blob = b"".join(handles)
        if len(blob) != 64 * self.nranks:
            raise ValueError("need one 64-byte handle per rank")
        _check(load().ppcx_xchg_connect(self._h, blob))

    @staticmethod
    def local_group(n, max_chains, devices=None):
        xs = [Xchg(n, k, max_chains, device=(devices[k] if devices else 0)) for k in range(n)]
        arr = (C.c_void_p * n)(*[x._h for x in xs])
        _check(load().ppcx_xchg_connect_local(arr, n))
        return xs

    def set_timeout(self, seconds):
        _check(load().ppcx_xchg_set_timeout(self._h, float(seconds)))

    def close(self):
        if getattr(self, "_h", None):
            load().ppcx_xchg_destroy(self._h)
            self._h = None


@dataclass
class Timing:
    seconds: float
    grad_evals: int
    gene_kernel_ms_mean: float
    gene_kernel_samples: int
    gene_kernel_chain_launches_mean: float


class Fit:
    """Kept draws + diagnostics of one NUTS run, resident on the device."""

    def __init__(self, model: Model, handle):
        self.model, self._h = model, handle
        c, k, d, it = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(load().ppcx_fit_info(handle, C.byref(c), C.byref(k), C.byref(d), C.byref(it)))
        self.chains, self.n_keep, self.D, self.iter = c.value, k.value, d.value, it.value

    def draws(self):
        out = np.zeros((self.chains, self.n_keep, self.D))
        _check(load().ppcx_fit_get_draws(self._h, _p(out, C.c_double)))
        return out

    def columns(self, cols):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        out = np.zeros((self.chains, self.n_keep, cols.size))
        _check(load().ppcx_fit_get_columns(self._h, int(cols.size), _p(cols, C.c_int32), _p(out, C.c_double)))
        return out

    def summary(self, cols=None, lp=True):
        """Per-column summary on the device (include/ppcx.h ppcx_fit_summary; rstan::monitor): a dict of 1-D float64 arrays
        mean, sd, q05, q50, q95, rhat, ess_bulk, ess_tail, and `column` (the column index, -1 for lp__). cols=None: all D
        columns; lp: lp__ last."""
        cols = np.arange(self.D) if cols is None else np.asarray(cols, dtype=np.int64).ravel()
        cols = np.ascontiguousarray(np.concatenate([cols, [-1]]) if lp else cols, dtype=np.int32)
        out = np.zeros((cols.size, len(SUMMARY_FIELDS)))
        if cols.size:
            _check(load().ppcx_fit_summary(self._h, int(cols.size), _p(cols, C.c_int32), _p(out, C.c_double)))
        res = {k: out[:, i].copy() for i, k in enumerate(SUMMARY_FIELDS)}
        res["column"] = cols.astype(np.int64)
        return res

    def approximation(self):
        """(mu, omega) of an ADVI fit's mean-field approximation, D values each (include/ppcx.h ppcx_fit_get_approximation)."""
        mu, om = np.zeros(self.D), np.zeros(self.D)
        _check(load().ppcx_fit_get_approximation(self._h, _p(mu, C.c_double), _p(om, C.c_double)))
        return mu, om

    def log_ratios(self):
        """(log_p, log_g) at each kept draw of an ADVI fit (ppcx_fit_get_log_ratios); the log ratios are log_p - log_g."""
        lp, lg = np.zeros(self.n_keep), np.zeros(self.n_keep)
        _check(load().ppcx_fit_get_log_ratios(self._h, _p(lp, C.c_double), _p(lg, C.c_double)))
        return lp, lg

    def psis(self, cols=None, overall=True):
        """Pareto-k diagnostic of an ADVI fit on the device (ppcx_fit_psis; what rstan::vb reports): a dict of `khat` and
        `column` (the column index, -1 for the log ratios themselves). cols=None: all D columns; overall: the k-hat of the log
        ratios last, as column -1."""
        cols = np.arange(self.D) if cols is None else np.asarray(cols, dtype=np.int64).ravel()
        cols = np.ascontiguousarray(np.concatenate([cols, [-1]]) if overall else cols, dtype=np.int32)
        out = np.zeros(cols.size)
        if cols.size:
            _check(load().ppcx_fit_psis(self._h, int(cols.size), _p(cols, C.c_int32), _p(out, C.c_double)))
        return {"khat": out, "column": cols.astype(np.int64)}

    def _genes(self, genes):
        G = self.model.G
        g = np.arange(G) if genes is None else np.asarray(genes, dtype=np.int64).ravel()
        return np.ascontiguousarray(g, dtype=np.int32)

    def log_lik(self, genes=None):
        """The cells' log-likelihood at every kept draw (include/ppcx.h ppcx_fit_get_log_lik; what a Stan log_lik block holds):
        [chains, n_keep, n_genes, S]. genes=None: all G genes. Excluded cells hold theirs too."""
        g = self._genes(genes)
        out = np.zeros((self.chains, self.n_keep, g.size, self.model.S))
        if g.size:
            _check(load().ppcx_fit_get_log_lik(self._h, int(g.size), _p(g, C.c_int32), _p(out, C.c_double)))
        return out

    def relative_eff(self, genes=None):
        """The relative efficiency of the importance ratios per observed cell on the device (ppcx_fit_relative_eff;
        loo::relative_eff(exp(log_lik), chain_id), what rstan::loo(fit) passes to loo::loo): [n_genes, S]. NaN where it is not
        defined (a NaN or +Inf log-likelihood, fewer than 4 kept draws per chain, no variance). genes=None: all G genes."""
        g = self._genes(genes)
        out = np.zeros((g.size, self.model.S))
        if g.size:
            _check(load().ppcx_fit_relative_eff(self._h, int(g.size), _p(g, C.c_int32), _p(out, C.c_double)))
        return out

    def _r_eff(self, g, r_eff):
        """The r_eff argument of loo / loo_predict as a contiguous [n_genes, S] array or None; "auto": relative_eff of the same
        genes with 1 where it is not defined (the default tail)."""
        if r_eff is None:
            return None
        if isinstance(r_eff, str):
            if r_eff != "auto":
                raise ValueError(f'r_eff must be None, "auto" or an array, not {r_eff!r}')
            re = self.relative_eff(g)
            return np.ascontiguousarray(np.where(np.isnan(re), 1.0, re))
        return np.ascontiguousarray(np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (g.size, self.model.S)))

    def _loo_cells(self, genes, r_eff, fields, call):
        """What loo and loo_predict share: call(n_genes, genes, r_eff or None, out) fills [n_genes, S, fields]. Returns the
        genes, the dict of the fields and `excluded`, and what closes the dict after the caller's own keys: `genes`, `n_draws`
        and, for r_eff="auto", the `r_eff` that was used."""
        g = self._genes(genes)
        S = self.model.S
        out = np.zeros((g.size, S, len(fields)))
        re = self._r_eff(g, r_eff)
        if g.size:
            _check(call(int(g.size), _p(g, C.c_int32), _p(re, C.c_double), _p(out, C.c_double)))
        res = {k: out[:, :, i].copy() for i, k in enumerate(fields)}
        excl = np.zeros(self.model.G * S, bool)
        excl[np.asarray(self.model.excl, dtype=np.int64)] = True
        res["excluded"] = excl.reshape(self.model.G, S)[g]
        last = {"genes": g.astype(np.int64), "n_draws": self.chains * self.n_keep}
        if isinstance(r_eff, str):
            last["r_eff"] = re
        return g, res, last

    def loo(self, genes=None, r_eff=None, mcse=False):
        """PSIS-LOO per observed cell on the device (ppcx_fit_loo; rstan::loo / loo::loo(log_lik, r_eff)): a dict of the
        pointwise elpd_loo, p_loo, looic and khat, [n_genes, S] each, `excluded` (the cells the model holds out now: elpd_loo is
        their exact held-out density, p_loo 0, khat NaN), `genes`, `n_draws`, and `estimates`: {elpd_loo, p_loo, looic: (sum, se)} over the
        non-excluded cells as loo reports them. genes=None: all G genes; r_eff None (all 1), [n_genes, S], or "auto": relative_eff
        of the same cells (1 where it is NaN), as rstan::loo(fit) does; the result then carries it as `r_eff`.
        mcse=True (ppcx_fit_loo_mcse; the fields above are the same bits): also loo's pointwise `mcse_elpd_loo` (the Monte-Carlo
        standard error of the cell's elpd_loo) and `n_eff` (the effective sample size of its PSIS weights; N r_eff for an
        excluded cell), [n_genes, S] each, and `mcse_elpd_loo_total` (inference.loo_mcse_total: loo's mcse_loo)."""
        entry = load().ppcx_fit_loo_mcse if mcse else load().ppcx_fit_loo
        _, res, last = self._loo_cells(genes, r_eff, LOO_MCSE_FIELDS if mcse else LOO_FIELDS,
                                       lambda n, g, re, out: entry(self._h, n, g, re, out))
        res.update(last)
        res["estimates"] = loo_estimates(res, res["excluded"])
        if mcse:
            from .inference import loo_mcse_total
            res["mcse_elpd_loo_total"] = loo_mcse_total(res)
        return res

    def loo_moment_match(self, genes=None, r_eff=None, k_threshold=None, max_iters=30, split=False, cov=False):
        """Fit.loo with gene-local moment matching of the cells whose khat exceeds k_threshold (ppcx_fit_loo_moment_match; the
        importance-weighted moment matching of loo::loo_moment_match, applied to the coordinates of the cell's own gene only --
        a deliberate deviation, restated from the paper and not run against R): Fit.loo's dict with `estimates` over the new
        values, plus `khat_before` (plain PSIS's khat; `khat` is the final one), `iterations` (accepted steps, int64), `scale`
        and `shift` [n_genes, S, C + 1] (the matched draws of the gene are scale * draw + shift, rows intercept, slopes,
        sigma_raw; 1 and 0 for a row the gene does not have) and `k_threshold`. A cell with iterations == 0 holds Fit.loo's
        bits. k_threshold=None: inference.loo_threshold(n_draws). Without the keywords below there is no covariance step and no
        split transformation: a matched khat is necessary, not sufficient; no mcse / n_eff. Not for an ADVI fit
        (Fit.loo_moment_match_approximate_posterior). r_eff as Fit.loo.
        split=True (ppcx_fit_loo_moment_match_split): the split transformation of loo::loo_moment_match on the matched cells --
        the first n_draws // 2 draws in the fit's order (whole leading chains) are transformed, the others kept, and all are
        weighted against the mixture they come from, so elpd_loo, p_loo, looic and `estimates` no longer rest on the matched
        draws being a sample of a known density. `khat`, `khat_before`, `iterations`, `scale` and `shift` stay the matching's
        bits; added are `elpd_loo_matched` (the elpd_loo of split=False) and `khat_split` (the k-hat of the split ratios, a
        diagnostic, NaN where iterations == 0).
        cov=True (ppcx_fit_loo_moment_match_cov; restated from the paper and the published package, not run against R): the
        covariance step as a third candidate, tried when the shift is refused and the scale is refused or invalid -- the gene's
        draws are mapped so that their mean and covariance over its coordinates become the weighted ones. The state is then an
        affine map: in place of `scale` the dict has `transform` [n_genes, S, C + 1, C + 1] (the matched draws are
        transform @ draw + shift; a row or column the gene does not have is the identity's) and `cov_iterations` (the accepted
        steps of that kind, int64); with split=True also `elpd_loo_matched` and `khat_split` as above. The predictive under these
        weights is Fit.loo_predict_exact_moment_match_cov. Still left out: mcse / n_eff of a matched cell, the covariance
        step for ADVI fits."""
        if k_threshold is None:
            from .inference import loo_threshold
            k_threshold = loo_threshold(self.chains * self.n_keep)
        k_threshold, max_iters = float(k_threshold), int(max_iters)
        nc = self.model.C + 1
        if cov:
            fields = LOO_MM_COV_HEAD + tuple(f"transform{c}" for c in range(nc * nc)) + tuple(f"shift{c}" for c in range(nc))
            _, res, last = self._loo_cells(genes, r_eff, fields, lambda n, g, re, out: load().ppcx_fit_loo_moment_match_cov(
                self._h, n, g, re, k_threshold, max_iters, int(bool(split)), out))
            tr = np.stack([res.pop(f"transform{c}") for c in range(nc * nc)], axis=-1)
            res["transform"] = tr.reshape(tr.shape[:-1] + (nc, nc))
            if not split:
                for name in LOO_MM_SPLIT_TAIL:
                    del res[name]
        else:
            fields = LOO_MM_HEAD + tuple(f"scale{c}" for c in range(nc)) + tuple(f"shift{c}" for c in range(nc))
            if split:
                fields = fields + LOO_MM_SPLIT_TAIL
            entry = load().ppcx_fit_loo_moment_match_split if split else load().ppcx_fit_loo_moment_match
            _, res, last = self._loo_cells(genes, r_eff, fields, lambda n, g, re, out: entry(
                self._h, n, g, re, k_threshold, max_iters, out))
            res["scale"] = np.stack([res.pop(f"scale{c}") for c in range(nc)], axis=-1)
        res["shift"] = np.stack([res.pop(f"shift{c}") for c in range(nc)], axis=-1)
        for name in ("iterations", "cov_iterations") if cov else ("iterations",):
            res[name] = res[name].astype(np.int64)
        res["k_threshold"] = k_threshold
        res.update(last)
        res["estimates"] = loo_estimates(res, res["excluded"])
        return res

    def _loo_predict_result(self, g, res, last):
        """closes a predictive result: `y`, `outside`, then _loo_cells' last keys"""
        res["y"] = np.asarray(self.model.counts).reshape(self.model.G, self.model.S)[g].astype(np.int64)
        with np.errstate(invalid="ignore"):
            res["outside"] = (res["y"] < res["lower"]) | (res["y"] > res["upper"])
        res.update(last)
        return res

    def loo_predict(self, genes=None, r_eff=None, p_lo=0.025, p_hi=0.975, seed=1, truncation_compensation=1.0):
        """The leave-one-out predictive interval and LOO-PIT per observed cell on the device (ppcx_fit_loo_predict; loo::E_loo,
        bayesplot::ppc_loo_intervals / ppc_loo_pit): a dict of mean, lower, upper (the p_lo / p_hi quantiles of the cell's count
        under the posterior that has not seen the cell), pit_lt, pit_le (P(x < y), P(x <= y)) and khat, [n_genes, S] each;
        `excluded` (cells the model holds out now: uniform weights, Fit.ppc's interval, khat NaN), `y` (the observed counts),
        `outside` = (y < lower) | (y > upper), `genes`, `n_draws`. genes=None: all G genes; r_eff as Fit.loo ("auto" adds `r_eff`).
        seed and truncation_compensation as Fit.ppc: the predictive counts of a checked gene are its counts_rng."""
        g, res, last = self._loo_cells(genes, r_eff, LOO_PREDICT_FIELDS, lambda n, g, re, out: load().ppcx_fit_loo_predict(
            self._h, n, g, re, float(truncation_compensation), float(p_lo), float(p_hi), int(seed), out))
        return self._loo_predict_result(g, res, last)

    def loo_approximate_posterior(self, genes=None):
        """PSIS-LOO per observed cell of an ADVI fit on the device (ppcx_fit_loo_approx; loo::loo_approximate_posterior(log_lik,
        log_p, log_g)): Fit.loo's dict -- the pointwise elpd_loo, p_loo, looic and khat, [n_genes, S] each, `excluded`, `genes`,
        `n_draws`, `estimates` over the non-excluded cells -- and `khat_approximation`, the overall k-hat of the approximation
        (Fit.psis, column -1). The ratios are (log_p - log_g) - log_lik, r_eff = 1. An excluded cell is held out of p already but
        still needs the correction for g: elpd_loo under the weights of log_p - log_g, p_loo 0, khat = khat_approximation.
        genes=None: all G genes. Not for a NUTS fit (Fit.loo); no mcse / n_eff."""
        _, res, last = self._loo_cells(genes, None, LOO_FIELDS, lambda n, g, re, out: load().ppcx_fit_loo_approx(self._h, n, g, out))
        res.update(last)
        res["estimates"] = loo_estimates(res, res["excluded"])
        res["khat_approximation"] = float(self.psis(cols=[], overall=True)["khat"][-1])
        return res

    def loo_moment_match_approximate_posterior(self, genes=None, k_threshold=None, max_iters=30):
        """Fit.loo_approximate_posterior with gene-local moment matching of the cells whose khat exceeds k_threshold
        (ppcx_fit_loo_moment_match_approx): Fit.loo_moment_match's construction for draws that come from the approximation of an
        ADVI fit -- a candidate's log ratios are (log_p - log_g) plus those of Fit.loo_moment_match, on the cached array of Fit.psis
        (loo::loo_moment_match has no approximate-posterior form: a deliberate deviation, restated from Paananen et al. 2021 and
        Magnusson et al. 2019, not run against R). Fit.loo_moment_match's dict -- `estimates` over the new values, `khat_before`,
        `iterations` (int64), `scale` and `shift` [n_genes, S, C + 1], `k_threshold` -- plus `khat_approximation`. A cell with
        iterations == 0 holds Fit.loo_approximate_posterior's bits. k_threshold=None: inference.loo_threshold(n_draws). Left out:
        the split transformation, the covariance step, mcse / n_eff. A matched khat below the threshold is necessary, not
        sufficient; and where `khat_approximation` is itself above the threshold the mismatch sits in the hyper-parameters as
        well, which a gene's own coordinates cannot repair. Not for a NUTS fit (Fit.loo_moment_match)."""
        if k_threshold is None:
            from .inference import loo_threshold
            k_threshold = loo_threshold(self.chains * self.n_keep)
        k_threshold, max_iters = float(k_threshold), int(max_iters)
        nc = self.model.C + 1
        fields = LOO_MM_HEAD + tuple(f"scale{c}" for c in range(nc)) + tuple(f"shift{c}" for c in range(nc))
        _, res, last = self._loo_cells(genes, None, fields, lambda n, g, re, out: load().ppcx_fit_loo_moment_match_approx(
            self._h, n, g, k_threshold, max_iters, out))
        res["scale"] = np.stack([res.pop(f"scale{c}") for c in range(nc)], axis=-1)
        res["shift"] = np.stack([res.pop(f"shift{c}") for c in range(nc)], axis=-1)
        res["iterations"] = res["iterations"].astype(np.int64)
        res["k_threshold"] = k_threshold
        res.update(last)
        res["estimates"] = loo_estimates(res, res["excluded"])
        res["khat_approximation"] = float(self.psis(cols=[], overall=True)["khat"][-1])
        return res

    def loo_predict_approximate_posterior(self, genes=None, p_lo=0.025, p_hi=0.975, seed=1, truncation_compensation=1.0):
        """The leave-one-out predictive interval and LOO-PIT per observed cell of an ADVI fit on the device
        (ppcx_fit_loo_predict_approx): Fit.loo_predict's dict (without r_eff) under the weights of loo_approximate_posterior. An
        excluded cell is weighted too (by log_p - log_g), so its interval is not Fit.ppc's; its khat is the overall k-hat."""
        g, res, last = self._loo_cells(genes, None, LOO_PREDICT_FIELDS, lambda n, g, re, out: load().ppcx_fit_loo_predict_approx(
            self._h, n, g, float(truncation_compensation), float(p_lo), float(p_hi), int(seed), out))
        return self._loo_predict_result(g, res, last)

    def ppc_exact(self, genes=None, p_lo=0.025, p_hi=0.975, truncation_compensation=1.0):
        """The exact posterior-predictive tail probabilities and interval per cell of checked genes on the device
        (ppcx_fit_ppc_exact): the predictive cdf of a cell is the average over the kept draws of negative-binomial cdfs, so nothing
        is sampled -- what Fit.ppc estimates from one drawn count per draw. NUTS, ADVI and fit_from_draws fits. A dict of
        [n_genes, S] arrays: mean, sd, p_le = P(X <= y), p_ge = P(X >= y) (floats), lower, upper (integers: the smallest k with
        F(k) >= p_lo, p_hi -- the distribution's inverse-cdf quantiles, where Fit.ppc reports type-7 sample quantiles that
        interpolate between integers; the two agree in the limit of draws), y (integers), excluded, outside = (y < lower) |
        (y > upper) (booleans), and `genes`, `n_draws`. A cell with an invalid draw: NaN floats, lower = upper = -1, outside
        False. genes=None: all K checked genes; ids are those of checked genes (0 .. K - 1)."""
        g = np.ascontiguousarray(np.arange(self.model.K) if genes is None else np.asarray(genes, dtype=np.int64).ravel(), dtype=np.int32)
        out = np.zeros((g.size, self.model.S, len(PPC_EXACT_FIELDS)))
        if g.size:
            _check(load().ppcx_fit_ppc_exact(self._h, int(g.size), _p(g, C.c_int32), float(truncation_compensation), float(p_lo),
                                             float(p_hi), _p(out, C.c_double)))
        res = _ppc_exact_dict(out)
        res["genes"] = g.astype(np.int64)
        res["n_draws"] = self.chains * self.n_keep
        return res

    def _loo_exact(self, genes, r_eff, call, more=0, tail=None):
        """What the exact leave-one-out forms share: call(n_genes, genes, r_eff or None, out) fills [n_genes, S, 10 + more];
        tail(res, the `more` fields behind the ten) adds a form's own keys"""
        g = np.ascontiguousarray(np.arange(self.model.K) if genes is None else np.asarray(genes, dtype=np.int64).ravel(), dtype=np.int32)
        out = np.zeros((g.size, self.model.S, len(LOO_EXACT_FIELDS) + more))
        re = self._r_eff(g, r_eff)
        if g.size:
            _check(call(int(g.size), _p(g, C.c_int32), _p(re, C.c_double), _p(out, C.c_double)))
        res = _loo_exact_dict(out)
        if tail is not None:
            tail(res, out[..., len(LOO_EXACT_FIELDS):])
        res["genes"] = g.astype(np.int64)
        res["n_draws"] = self.chains * self.n_keep
        if isinstance(r_eff, str):
            res["r_eff"] = re
        return res

    def loo_predict_exact(self, genes=None, r_eff=None, p_lo=0.025, p_hi=0.975, truncation_compensation=1.0):
        """The exact leave-one-out predictive tail probabilities and interval per cell of checked genes of a NUTS fit on the device
        (ppcx_fit_loo_predict_exact): the predictive cdf of a cell under the posterior that has not seen it is the average of the
        draws' negative-binomial cdfs under Fit.loo_predict's PSIS weights, so nothing is sampled -- what Fit.loo_predict
        estimates from one drawn count per draw (in R: loo::E_loo on exact cdfs; restated from the published definitions, not
        run against R). Fit.ppc_exact's dict of [n_genes, S] arrays (mean, sd, p_le, p_ge, lower, upper, y, excluded, outside,
        `genes`, `n_draws`) under those weights, plus khat (Fit.loo_predict's, bit for bit) and the two ends of the randomised
        LOO-PIT, pit_lt = 1 - p_ge and pit_le = p_le. A cell the model excludes is already held out: Fit.ppc_exact's values,
        khat NaN. genes=None: all K checked genes (ids 0 .. K - 1); r_eff as Fit.loo_predict ("auto" adds `r_eff`)."""
        return self._loo_exact(genes, r_eff, lambda n, g, re, out: load().ppcx_fit_loo_predict_exact(
            self._h, n, g, re, float(truncation_compensation), float(p_lo), float(p_hi), out))

    def loo_predict_exact_moment_match(self, genes=None, r_eff=None, k_threshold=None, max_iters=30, p_lo=0.025, p_hi=0.975,
                                       truncation_compensation=1.0, split=False):
        """Fit.loo_predict_exact with gene-local moment matching of the cells whose khat exceeds k_threshold
        (ppcx_fit_loo_predict_exact_moment_match): the outlying cells, whose plain PSIS weights are not to be trusted, are matched
        as Fit.loo_moment_match matches them, and their predictive is importance sampling with the matched draws as the proposal
        -- the weights are PSIS on the ratios of the local density, the negative binomials are evaluated at the matched draws;
        nothing is sampled. Fit.loo_predict_exact's dict (`khat` is the final one), plus Fit.loo_moment_match's `khat_before`,
        `iterations` (int64), `scale` and `shift` [n_genes, S, C + 1] (the same bits as that method's) and `k_threshold`. A cell
        with iterations == 0 holds Fit.loo_predict_exact's bits. k_threshold=None: inference.loo_threshold(n_draws). No covariance
        step (Fit.loo_predict_exact_moment_match_cov has it) and no split transformation: a matched khat is necessary, not
        sufficient. Not for an ADVI fit (Fit.loo_predict_exact_moment_match_approximate_posterior).
        split=True (ppcx_fit_loo_predict_exact_moment_match_split): the split transformation as in Fit.loo_moment_match -- the
        negative binomials are evaluated at the matched draws for the first n_draws // 2 draws in the fit's order and at the
        original draws for the others, under the PSIS weights of the split ratios. `khat` and the matching's record stay its
        bits; added is `khat_split` (NaN where iterations == 0)."""
        if k_threshold is None:
            from .inference import loo_threshold
            k_threshold = loo_threshold(self.chains * self.n_keep)
        k_threshold, max_iters = float(k_threshold), int(max_iters)
        nc = self.model.C + 1

        def tail(res, more):
            res["khat_before"] = more[..., 0].copy()
            res["iterations"] = more[..., 1].astype(np.int64)
            res["scale"] = more[..., 2:2 + nc].copy()
            res["shift"] = more[..., 2 + nc:2 + 2 * nc].copy()
            res["k_threshold"] = k_threshold
            if split:
                res["khat_split"] = more[..., 2 + 2 * nc].copy()
        entry = load().ppcx_fit_loo_predict_exact_moment_match_split if split else load().ppcx_fit_loo_predict_exact_moment_match
        return self._loo_exact(genes, r_eff, lambda n, g, re, out: entry(
            self._h, n, g, re, k_threshold, max_iters, float(truncation_compensation), float(p_lo), float(p_hi), out),
            more=2 + 2 * nc + (1 if split else 0), tail=tail)

    def loo_predict_exact_moment_match_cov(self, genes=None, r_eff=None, k_threshold=None, max_iters=30, p_lo=0.025, p_hi=0.975,
                                           truncation_compensation=1.0, split=False):
        """Fit.loo_predict_exact with the cells whose khat exceeds k_threshold matched first as Fit.loo_moment_match(cov=True)
        matches them (ppcx_fit_loo_predict_exact_moment_match_cov; restated from the paper and the published package, not run
        against R): the predictive is taken under those weights at the affinely matched draws transform @ draw + shift; nothing
        is sampled. Fit.loo_predict_exact's dict (`khat` is the final one), plus `khat_before`, `iterations` and
        `cov_iterations` (int64), `transform` [n_genes, S, C + 1, C + 1], `shift` [n_genes, S, C + 1] (the same bits as
        Fit.loo_moment_match(cov=True)'s) and `k_threshold`; there is no `scale`. A cell with iterations == 0 holds
        Fit.loo_predict_exact's bits. k_threshold=None: inference.loo_threshold(n_draws). Not for an ADVI fit; no mcse / n_eff of
        a matched cell.
        split=True: the split transformation on the affine map -- the negative binomials are evaluated at the matched draws for
        the first n_draws // 2 draws in the fit's order and at the original draws for the others, under the PSIS weights of the
        split ratios of Fit.loo_moment_match(cov=True, split=True). `khat` and the matching's record stay its bits; added is
        `khat_split` (NaN where iterations == 0)."""
        if k_threshold is None:
            from .inference import loo_threshold
            k_threshold = loo_threshold(self.chains * self.n_keep)
        k_threshold, max_iters = float(k_threshold), int(max_iters)
        nc = self.model.C + 1

        def tail(res, more):
            res["khat_before"] = more[..., 0].copy()
            res["iterations"] = more[..., 1].astype(np.int64)
            res["cov_iterations"] = more[..., 2].astype(np.int64)
            res["transform"] = more[..., 4:4 + nc * nc].reshape(more.shape[:-1] + (nc, nc)).copy()
            res["shift"] = more[..., 4 + nc * nc:4 + nc * nc + nc].copy()
            res["k_threshold"] = k_threshold
            if split:
                res["khat_split"] = more[..., 3].copy()
        return self._loo_exact(genes, r_eff, lambda n, g, re, out: load().ppcx_fit_loo_predict_exact_moment_match_cov(
            self._h, n, g, re, k_threshold, max_iters, int(bool(split)), float(truncation_compensation), float(p_lo), float(p_hi), out),
            more=4 + nc * nc + nc, tail=tail)

    def loo_predict_exact_approximate_posterior(self, genes=None, p_lo=0.025, p_hi=0.975, truncation_compensation=1.0):
        """Fit.loo_predict_exact for an ADVI fit (ppcx_fit_loo_predict_exact_approx): the same dict (without r_eff) under the
        weights of loo_approximate_posterior, and `khat_approximation`, the overall k-hat of the approximation. An excluded cell
        is weighted too (by log_p - log_g); its khat is the overall k-hat."""
        res = self._loo_exact(genes, None, lambda n, g, re, out: load().ppcx_fit_loo_predict_exact_approx(
            self._h, n, g, float(truncation_compensation), float(p_lo), float(p_hi), out))
        res["khat_approximation"] = float(self.psis(cols=[], overall=True)["khat"][-1])
        return res

    def loo_predict_exact_moment_match_approximate_posterior(self, genes=None, k_threshold=None, max_iters=30, p_lo=0.025, p_hi=0.975,
                                                             truncation_compensation=1.0):
        """Fit.loo_predict_exact_approximate_posterior with the cells whose khat exceeds k_threshold matched first as
        Fit.loo_moment_match_approximate_posterior matches them (ppcx_fit_loo_predict_exact_moment_match_approx): their predictive
        is taken under the matched weights with the negative binomials evaluated at the matched draws; nothing is sampled.
        Fit.loo_predict_exact_approximate_posterior's dict (`khat` is the final one; `khat_approximation`), plus `khat_before`,
        `iterations` (int64), `scale` and `shift` [n_genes, S, C + 1] (the same bits as that method's) and `k_threshold`. A cell
        with iterations == 0 holds Fit.loo_predict_exact_approximate_posterior's bits. What is left out, and what a matched khat
        does not say, as Fit.loo_moment_match_approximate_posterior. Not for a NUTS fit (Fit.loo_predict_exact_moment_match)."""
        if k_threshold is None:
            from .inference import loo_threshold
            k_threshold = loo_threshold(self.chains * self.n_keep)
        k_threshold, max_iters = float(k_threshold), int(max_iters)
        nc = self.model.C + 1

        def tail(res, more):
            res["khat_before"] = more[..., 0].copy()
            res["iterations"] = more[..., 1].astype(np.int64)
            res["scale"] = more[..., 2:2 + nc].copy()
            res["shift"] = more[..., 2 + nc:2 + 2 * nc].copy()
            res["k_threshold"] = k_threshold
        res = self._loo_exact(genes, None, lambda n, g, re, out: load().ppcx_fit_loo_predict_exact_moment_match_approx(
            self._h, n, g, k_threshold, max_iters, float(truncation_compensation), float(p_lo), float(p_hi), out),
            more=2 + 2 * nc, tail=tail)
        res["khat_approximation"] = float(self.psis(cols=[], overall=True)["khat"][-1])
        return res

    def diagnostics(self):
        lp = np.zeros((self.chains, self.n_keep))
        ss = np.zeros((self.chains, self.iter))
        acc = np.zeros((self.chains, self.iter))
        td = np.zeros((self.chains, self.iter), np.int32)
        nl = np.zeros((self.chains, self.iter), np.int32)
        dv = np.zeros((self.chains, self.iter), np.int32)
        _check(load().ppcx_fit_get_diagnostics(self._h, _p(lp, C.c_double), _p(ss, C.c_double), _p(td, C.c_int32),
                                                _p(nl, C.c_int32), _p(dv, C.c_int32), _p(acc, C.c_double)))
        return dict(lp=lp, stepsize=ss, treedepth=td, n_leapfrog=nl, divergent=dv, accept=acc)

    def inv_metric(self):
        """[chains, D] diagonal of the adapted inverse metric (rstan::get_adaptation_info)."""
        out = np.zeros((self.chains, self.D))
        _check(load().ppcx_fit_get_inv_metric(self._h, _p(out, C.c_double)))
        return out

    def timing(self) -> Timing:
        s, ms, cl = C.c_double(), C.c_double(), C.c_double()
        ge, ns = C.c_longlong(), C.c_longlong()
        _check(load().ppcx_fit_get_timing(self._h, C.byref(s), C.byref(ge), C.byref(ms), C.byref(ns), C.byref(cl)))
        return Timing(s.value, ge.value, ms.value, ns.value, cl.value)

    def advi_info(self):
        it, cv = C.c_int(), C.c_int()
        el, et = C.c_double(), C.c_double()
        _check(load().ppcx_fit_advi_info(self._h, C.byref(it), C.byref(cv), C.byref(el), C.byref(et)))
        return dict(iterations=it.value, converged=bool(cv.value), elbo=el.value, eta=et.value)

    def xchg_timing(self):
        """(mean us a chain's state machine waited for its peers per exchange, exchanges) of a direct-exchange fit."""
        us, n = C.c_double(), C.c_longlong()
        _check(load().ppcx_fit_get_xchg_timing(self._h, C.byref(us), C.byref(n)))
        return us.value, int(n.value)

    def ppc_timing(self):
        """(kernel ms, NB draws) of the last ppc() call on this fit."""
        ms, n = C.c_double(), C.c_longlong()
        _check(load().ppcx_fit_get_ppc_timing(self._h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def kernel_times(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        n = C.c_longlong()
        _check(load().ppcx_fit_get_kernel_times(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(loglik_ms=a.value, close_ms=b.value, update_ms=c.value, launch_triples=n.value)

    def ppc(self, truncation_compensation=1.0, p_lo=0.025, p_hi=0.975, seed=1, n_gen=0, resample=False,
            return_counts_rng=False):
        K, S = self.model.K, self.model.S
        ci = np.zeros((K, S, 4))
        n = n_gen if n_gen > 0 else self.chains * self.n_keep
        rng = np.zeros((n, K, S), np.int32) if return_counts_rng else None
        _check(load().ppcx_fit_ppc(self._h, float(truncation_compensation), float(p_lo), float(p_hi), int(seed),
                                   int(n_gen), int(bool(resample)), _p(ci, C.c_double), _p(rng, C.c_int32)))
        return (ci, rng) if return_counts_rng else ci

    def close(self):
        if getattr(self, "_h", None):
            load().ppcx_fit_free(self._h)
            self._h = None

    # a device-resident handle: copies (pandas deep-copies DataFrame.attrs, where identify_outliers(pass_fit=True) puts the
    # fits, R/methods.R:353-357) share it
    def __copy__(self):
        return self

    def __deepcopy__(self, memo):
        return self

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
