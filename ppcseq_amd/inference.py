"""Host-side mirror of ppcseq's inference driver `do_inference()` (R/utilities.R:1321-1547).

Same names, argument meaning and error behaviour as the reference for this path; the only thing
replaced is the sampler call: `rstan::sampling(stanmodels$negBinomial_MPI, ...)`
(R/utilities.R:1497-1512) becomes the C-ABI library `libppcx.so` (include/ppcx.h) driving HIP kernels
on the MI355X. The shard packing of the reference (`format_for_MPI` R/utilities.R:125-174,
`counts_package` :1452-1461) is a CPU-threading artefact and is not reproduced: the library takes the
logical G x S matrix. There is no CPU fallback.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, field

import numpy as np

from . import _lib


def find_optimal_number_of_chains(how_many_posterior_draws, max_number_to_check=100):
    """R/utilities.R:291-303: argmin over c in 2..max of draws/c + 150 c (first minimiser)."""
    best, best_tot = 2, float("inf")
    for c in range(2, max_number_to_check + 1):
        tot = how_many_posterior_draws / c + 150 * c
        if tot < best_tot:
            best, best_tot = c, tot
    return best


def quantile7(x, p):
    """R `quantile(type = 7)` (rstan::summary / stats::quantile default)."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    h = (x.size - 1) * p
    lo = int(math.floor(h))
    if lo >= x.size - 1:
        return float(x[-1])
    return float(x[lo] + (h - lo) * (x[lo + 1] - x[lo]))


@dataclass
class InferenceResult:
    """What `do_inference` returns, as arrays over the checked cells (g < K, all samples).

    Columns of the reference's tibble (R/utilities.R:1516-1544): S, G (1-based), mean, sd, .lower,
    .upper, ppc, `is higher than mean`, slope, `is group high`, deleterious_outliers.
    """
    K: int
    S: int
    mean: np.ndarray            # [K, S]
    sd: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    ppc: np.ndarray             # bool [K, S]
    is_higher_than_mean: np.ndarray
    slope: np.ndarray           # [K] posterior mean of alpha_sub_1
    is_group_high: np.ndarray | None
    deleterious_outliers: np.ndarray | None
    total_draws: int
    chains: int
    iter: int
    fit: object = None          # the device-resident Fit when pass_fit
    diagnostics: dict = field(default_factory=dict)
    counts_rng: np.ndarray | None = None
    convergence: dict | None = None   # check_convergence: Fit.summary of alpha_sub_1 (and lp__ where the fit holds it)
    approximation: dict | None = None  # check_approximation: Fit.psis of alpha_sub_1 and the overall k-hat (column -1, last)
    loo: dict | None = None            # check_loo: Fit.loo of the checked genes' cells ([K, S] arrays and loo's estimates)
    loo_intervals: dict | None = None  # check_loo_intervals: Fit.loo_predict of the checked genes' cells ([K, S] arrays)
    approximation_loo: dict | None = None            # check_approximation_loo: Fit.loo_approximate_posterior of those cells
    exact_intervals: dict | None = None  # exact_intervals: Fit.ppc_exact of the checked genes' cells ([K, S] arrays)
    approximation_loo_intervals: dict | None = None  # check_approximation_loo_intervals: Fit.loo_predict_approximate_posterior
    exact_loo_intervals: dict | None = None  # exact_loo_intervals: Fit.loo_predict_exact of the checked genes' cells ([K, S] arrays)
    exact_approximation_loo_intervals: dict | None = None  # ...: Fit.loo_predict_exact_approximate_posterior of those cells

    def to_frame(self):
        import pandas as pd
        K, S = self.K, self.S
        g, s = np.meshgrid(np.arange(1, K + 1), np.arange(1, S + 1), indexing="ij")
        d = {"S": s.ravel(), "G": g.ravel(), "mean": self.mean.ravel(), "sd": self.sd.ravel(),
             ".lower": self.lower.ravel(), ".upper": self.upper.ravel(), "ppc": self.ppc.ravel(),
             "is higher than mean": self.is_higher_than_mean.ravel(), "slope": np.repeat(self.slope, S)}
        if self.deleterious_outliers is not None:
            d["is group high"] = self.is_group_high.ravel()
            d["deleterious_outliers"] = self.deleterious_outliers.ravel()
        return pd.DataFrame(d)


def hmc_warnings(diagnostics, warmup, max_treedepth=10):
    """What rstan::sampling tells the reference's user after a NUTS fit (check_hmc_diagnostics: divergent transitions after
    warm-up, transitions that hit the maximum tree depth), as a list of messages. A chain that ends the short warm-up of the
    reference (150 iterations, R/utilities.R:1503) with a step size far below the others' runs every transition at the
    maximum tree depth -- the fit then takes several times as long and this is how the caller learns why."""
    msgs = []
    div = np.asarray(diagnostics["divergent"])[:, warmup:]
    depth = np.asarray(diagnostics["treedepth"])[:, warmup:]
    if div.size and div.sum() > 0:
        msgs.append(f"There were {int(div.sum())} divergent transitions after warmup.")
    n_max = int((depth >= max_treedepth).sum()) if depth.size else 0
    if n_max > 0:
        chains = np.nonzero((depth >= max_treedepth).any(axis=1))[0].tolist()
        msgs.append(f"There were {n_max} transitions after warmup that exceeded the maximum treedepth of {max_treedepth} "
                    f"(chains {chains}): those chains adapted a very small step size and dominate the run time.")
    return msgs


RHAT_THRESHOLD = 1.05          # rstan::throw_sampler_warnings
ESS_PER_CHAIN = 100            # bulk / tail ESS below 100 x chains


def convergence_warnings(summary, chains):
    """What rstan::sampling adds after a fit (throw_sampler_warnings, rstan >= 2.21) from a summary of the saved parameters
    (Fit.summary): the largest rank-normalised R-hat above 1.05, a bulk or a tail ESS below 100 x chains. NaN entries (a column
    without variance) are ignored. Returns the messages, like hmc_warnings."""
    msgs = []
    rhat = np.asarray(summary["rhat"], dtype=np.float64)
    bulk = np.asarray(summary["ess_bulk"], dtype=np.float64)
    tail = np.asarray(summary["ess_tail"], dtype=np.float64)
    more = "Running the chains for more iterations may help. See\nhttps://mc-stan.org/misc/warnings.html"
    with np.errstate(invalid="ignore"):
        if np.any(rhat > RHAT_THRESHOLD):
            msgs.append(f"The largest R-hat is {round(float(np.nanmax(rhat)), 2)}, indicating chains have not mixed.\n{more}#r-hat")
        if np.any(bulk < ESS_PER_CHAIN * chains):
            msgs.append("Bulk Effective Samples Size (ESS) is too low, indicating posterior means and medians may be unreliable.\n"
                        f"{more}#bulk-ess")
        if np.any(tail < ESS_PER_CHAIN * chains):
            msgs.append("Tail Effective Samples Size (ESS) is too low, indicating posterior variances and tail quantiles may be "
                        f"unreliable.\n{more}#tail-ess")
    return msgs


KHAT_UNRELIABLE = 0.7          # rstan::vb: Pareto k above which resampling is unreliable
KHAT_DISABLED = 1.0            # ... and above which it is disabled


def approximation_warnings(khat):
    """What rstan::vb (rstan >= 2.21) tells its user about the quality of an ADVI fit from the Pareto k diagnostic of the log
    ratios log_p - log_g of its draws (Fit.psis): above 0.7 resampling is unreliable, above 1 it is disabled. `khat` is a number
    or an array (the largest non-NaN value is reported: do_inference passes the overall k-hat only, as rstan warns on it). NaN
    (a column with a non-finite draw) reports nothing. Returns the messages, like convergence_warnings."""
    k = np.asarray(khat, dtype=np.float64).ravel()
    k = k[~np.isnan(k)]
    if k.size == 0:
        return []
    top = float(k.max())
    shown = "Inf" if math.isinf(top) else f"{round(top, 2)}"
    if top > KHAT_DISABLED:
        return [f"Pareto k diagnostic value is {shown}. Resampling is disabled. Decreasing tol_rel_obj may help if variational "
                "algorithm has terminated prematurely. Otherwise consider using sampling instead."]
    if top > KHAT_UNRELIABLE:
        return [f"Pareto k diagnostic value is {shown}. Resampling is unreliable. Increasing the number of draws or decreasing "
                "tol_rel_obj may help."]
    return []


def loo_threshold(n_draws):
    """loo (>= 2.7): the Pareto k above which PSIS-LOO of an observation is unreliable at n_draws draws,
    min(1 - 1 / log10(n_draws), 0.7) -- 0.7 from 2 154 draws on"""
    return min(1.0 - 1.0 / math.log10(n_draws), 0.7)


def loo_warnings(khat, n_draws):
    """What loo tells its user after PSIS-LOO when any observation's k-hat exceeds loo_threshold(n_draws) (Fit.loo's khat,
    any shape; NaN -- an excluded cell or one with a non-finite log-likelihood -- reports nothing). Returns the messages, like
    convergence_warnings."""
    k = np.asarray(khat, dtype=np.float64).ravel()
    k = k[~np.isnan(k)]
    if k.size and float(k.max()) > loo_threshold(n_draws):
        return ["Some Pareto k diagnostic values are too high. See help('pareto-k-diagnostic') for details."]
    return []


def loo_mcse_total(loo):
    """loo's mcse_loo from Fit.loo(mcse=True): sqrt(sum mcse_elpd_loo^2) over the non-excluded cells, the Monte-Carlo standard
    error of their summed elpd_loo; NaN if any of their k-hats exceeds loo_threshold(n_draws) (the sum is then not to be
    trusted at all), or without such a cell."""
    keep = ~np.asarray(loo["excluded"], bool)
    k = np.asarray(loo["khat"], dtype=np.float64)[keep]
    if k.size == 0 or np.any(k[~np.isnan(k)] > loo_threshold(loo["n_draws"])):
        return float("nan")
    m = np.asarray(loo["mcse_elpd_loo"], dtype=np.float64)[keep]
    return float(np.sqrt(np.sum(m * m)))


def pareto_k_table(loo):
    """loo's pareto_k_table of a Fit.loo result, on the host: the non-excluded cells' k-hats (NaN ones left out) in the bins
    (-Inf, thr] (good), (thr, 1] (bad) and (1, Inf) (very bad), thr = loo_threshold(n_draws). Returns {"threshold", "bins":
    [{"label", "lower", "upper", "count", "pct", "min_n_eff"}, ...]}: pct in percent of the cells counted; min_n_eff the smallest
    n_eff of the bin's cells, NaN for an empty bin or a result without n_eff (Fit.loo(mcse=True) carries it)."""
    thr = loo_threshold(loo["n_draws"])
    keep = ~np.asarray(loo["excluded"], bool)
    k = np.asarray(loo["khat"], dtype=np.float64)[keep]
    ok = ~np.isnan(k)
    n_eff = np.asarray(loo["n_eff"], dtype=np.float64)[keep][ok] if "n_eff" in loo else None
    k = k[ok]
    bins = []
    for label, lo, hi in (("good", -np.inf, thr), ("bad", thr, 1.0), ("very bad", 1.0, np.inf)):
        inside = (k > lo) & (k <= hi) if lo != -np.inf else k <= hi
        cnt = int(inside.sum())
        mn = float(np.min(n_eff[inside])) if n_eff is not None and cnt else float("nan")
        bins.append(dict(label=label, lower=float(lo), upper=float(hi), count=cnt,
                         pct=100.0 * cnt / k.size if k.size else float("nan"), min_n_eff=mn))
    return dict(threshold=thr, bins=bins)


WARMUP = 150                   # R/utilities.R:1503


def pass_plan(how_many_posterior_draws, approximate_posterior_analysis, chains, cores):
    """(chains, n_iter, warmup) of one pass (R/utilities.R:1372-1386, :1502-1503): the chains as given, or what `cores` and the
    draws the fit has to keep allow."""
    draws_practical = 1000 if approximate_posterior_analysis else how_many_posterior_draws
    if chains is None:
        chains = max(3, min(int(cores), find_optimal_number_of_chains(draws_practical)))
    return chains, int(math.ceil(draws_practical / chains)) + WARMUP, WARMUP


# ---- the optional diagnostics of a pass: each stated once, here; do_inference's docstring says what they report

@dataclass
class CheckContext:
    """What the readers of the diagnostics need beside the fit."""
    K: int
    p: float                     # the pass's interval probabilities are p and 1 - p
    seed: int
    truncation_compensation: float
    loo_r_eff: object = None     # the modifiers of loo / loo_intervals
    loo_mcse: bool = False
    pooled: bool = False         # a fit over the pooled draws of several fits' chains (pooled_summary): it holds no lp__
    loo_moment_match: bool = False   # check_loo reads Fit.loo_moment_match in place of Fit.loo
    exact_loo_moment_match: bool = False   # exact_loo_intervals reads Fit.loo_predict_exact_moment_match in place of Fit.loo_predict_exact
    loo_moment_match_split: bool = False         # Fit.loo_moment_match is read with split=True
    exact_loo_moment_match_split: bool = False   # Fit.loo_predict_exact_moment_match is read with split=True
    loo_moment_match_cov: bool = False           # Fit.loo_moment_match is read with cov=True
    exact_loo_moment_match_cov: bool = False     # exact_loo_moment_match reads Fit.loo_predict_exact_moment_match_cov
    approximation_loo_moment_match: bool = False         # check_approximation_loo reads Fit.loo_moment_match_approximate_posterior
    exact_approximation_loo_moment_match: bool = False   # exact_approximation_loo_intervals reads
                                                         # Fit.loo_predict_exact_moment_match_approximate_posterior


@dataclass(frozen=True)
class Check:
    keyword: str                 # the option of do_inference / identify_outliers
    field: str                   # the InferenceResult field it fills; attrs["<field>_discovery"], ["<field>_test"] of the frame
    order: int                   # its place in the order of refusals (the order in which the options were added)
    kind: str | None             # the pass it needs: "nuts", "advi" or None (either)
    pooled: bool                 # available over pooled chains (devices=[...])
    ranks: bool                  # available to passes over several ranks (identify_outliers' _pass)
    refusal: str | None          # what the other kind of pass is told
    read: object                 # read(fit, ctx) -> dict
    warn: object = None          # warn(result, fit) -> messages
    cells: bool = True           # it reads the checked genes' cells: the pooled model then carries their exclusions, and
                                 # without a checked gene the pooled fit is not read (the field stays None)


def _alpha_sub_1(fit, K):
    return 3 + fit.model.G + np.arange(K)


def _interval(ctx):
    return dict(p_lo=ctx.p, p_hi=1 - ctx.p, truncation_compensation=ctx.truncation_compensation)


def _loo_warnings(result, fit):
    return loo_warnings(result["khat"], fit.chains * fit.n_keep)


def _read_loo(fit, ctx):
    """check_loo's read: Fit.loo(r_eff, mcse), or with loo_moment_match Fit.loo_moment_match(r_eff) (its khat is the final one),
    with loo_moment_match_split also split=True, with loo_moment_match_cov also cov=True"""
    if ctx.loo_moment_match:
        split = dict(split=True) if ctx.loo_moment_match_split else {}
        cov = dict(cov=True) if ctx.loo_moment_match_cov else {}
        return fit.loo_moment_match(np.arange(ctx.K), r_eff=ctx.loo_r_eff, **split, **cov)
    return fit.loo(np.arange(ctx.K), r_eff=ctx.loo_r_eff, mcse=bool(ctx.loo_mcse))


def _read_exact_loo(fit, ctx):
    """exact_loo_intervals' read: Fit.loo_predict_exact(r_eff, the pass's interval), or with exact_loo_moment_match
    Fit.loo_predict_exact_moment_match with the same keywords (its khat is the final one), with exact_loo_moment_match_split also
    split=True; with exact_loo_moment_match_cov the method is Fit.loo_predict_exact_moment_match_cov, its keywords the same"""
    read = fit.loo_predict_exact_moment_match if ctx.exact_loo_moment_match else fit.loo_predict_exact
    if ctx.exact_loo_moment_match and ctx.exact_loo_moment_match_cov:
        read = fit.loo_predict_exact_moment_match_cov
    split = dict(split=True) if ctx.exact_loo_moment_match and ctx.exact_loo_moment_match_split else {}
    return read(np.arange(ctx.K), r_eff=ctx.loo_r_eff, **_interval(ctx), **split)


def _read_approximation_loo(fit, ctx):
    """check_approximation_loo's read: Fit.loo_approximate_posterior, or with approximation_loo_moment_match
    Fit.loo_moment_match_approximate_posterior (its khat is the final one)"""
    read = fit.loo_moment_match_approximate_posterior if ctx.approximation_loo_moment_match else fit.loo_approximate_posterior
    return read(np.arange(ctx.K))


def _read_exact_approximation_loo(fit, ctx):
    """exact_approximation_loo_intervals' read: Fit.loo_predict_exact_approximate_posterior at the pass's interval, or with
    exact_approximation_loo_moment_match Fit.loo_predict_exact_moment_match_approximate_posterior with the same keywords"""
    read = (fit.loo_predict_exact_moment_match_approximate_posterior if ctx.exact_approximation_loo_moment_match
            else fit.loo_predict_exact_approximate_posterior)
    return read(np.arange(ctx.K), **_interval(ctx))


CHECKS = (          # in the order of the reads
    Check("check_approximation", "approximation", 2, "advi", False, False,
          "check_approximation needs an ADVI pass (approximate_posterior_inference = True): the Pareto k diagnostic judges the "
          "variational approximation",
          lambda fit, ctx: fit.psis(_alpha_sub_1(fit, ctx.K), overall=True),
          lambda result, fit: approximation_warnings(result["khat"][-1]), cells=False),
    Check("check_approximation_loo", "approximation_loo", 5, "advi", False, False,
          "check_approximation_loo needs an ADVI pass (approximate_posterior_inference = True): it corrects PSIS-LOO for the "
          "variational approximation; PSIS-LOO of a NUTS pass is check_loo",
          _read_approximation_loo, _loo_warnings),
    Check("check_approximation_loo_intervals", "approximation_loo_intervals", 6, "advi", False, False,
          "check_approximation_loo_intervals needs an ADVI pass (approximate_posterior_inference = True): the leave-one-out "
          "intervals of a NUTS pass are check_loo_intervals",
          lambda fit, ctx: fit.loo_predict_approximate_posterior(np.arange(ctx.K), seed=ctx.seed, **_interval(ctx))),
    Check("exact_approximation_loo_intervals", "exact_approximation_loo_intervals", 9, "advi", False, False,
          "exact_approximation_loo_intervals needs an ADVI pass (approximate_posterior_inference = True): the exact leave-one-out "
          "intervals of a NUTS pass are exact_loo_intervals",
          _read_exact_approximation_loo),
    Check("check_convergence", "convergence", 1, "nuts", True, False,
          "check_convergence needs a NUTS pass: the draws of an ADVI fit are independent (rstan::vb reports no R-hat or ESS)",
          lambda fit, ctx: fit.summary(_alpha_sub_1(fit, ctx.K), lp=not ctx.pooled),
          lambda result, fit: convergence_warnings(result, fit.chains), cells=False),
    Check("check_loo", "loo", 3, "nuts", True, False,
          "check_loo needs a NUTS pass: PSIS-LOO of an ADVI fit (loo_approximate_posterior) is check_approximation_loo",
          _read_loo, _loo_warnings),
    Check("check_loo_intervals", "loo_intervals", 4, "nuts", True, False,
          "check_loo_intervals needs a NUTS pass: the leave-one-out intervals of an ADVI fit (loo_approximate_posterior) are "
          "check_approximation_loo_intervals",
          lambda fit, ctx: fit.loo_predict(np.arange(ctx.K), r_eff=ctx.loo_r_eff, seed=ctx.seed, **_interval(ctx))),
    Check("exact_intervals", "exact_intervals", 7, None, True, False, None,
          lambda fit, ctx: fit.ppc_exact(np.arange(ctx.K), **_interval(ctx))),
    Check("exact_loo_intervals", "exact_loo_intervals", 8, "nuts", True, False,
          "exact_loo_intervals needs a NUTS pass: the exact leave-one-out intervals of an ADVI fit (loo_approximate_posterior) are "
          "exact_approximation_loo_intervals",
          _read_exact_loo),
)

MODIFIERS = (       # (option, the options of which it needs one, what it is told without one)
    ("loo_r_eff", ("check_loo", "check_loo_intervals", "exact_loo_intervals"),
     "loo_r_eff needs check_loo, check_loo_intervals or exact_loo_intervals: it is the r_eff of their PSIS"),
    ("loo_mcse", ("check_loo",),
     "loo_mcse needs check_loo: it adds the Monte-Carlo standard error and n_eff to its PSIS-LOO"),
    ("loo_moment_match", ("check_loo",),
     "loo_moment_match needs check_loo: it matches the moments of the cells whose k-hat its PSIS-LOO finds too high"),
    ("exact_loo_moment_match", ("exact_loo_intervals",),
     "exact_loo_moment_match needs exact_loo_intervals: it matches the moments of the cells whose k-hat their PSIS finds too high"),
    ("loo_moment_match_split", ("loo_moment_match",),
     "loo_moment_match_split needs loo_moment_match: it is the split transformation of the cells that it has matched"),
    ("exact_loo_moment_match_split", ("exact_loo_moment_match",),
     "exact_loo_moment_match_split needs exact_loo_moment_match: it is the split transformation of the cells that it has matched"),
    ("loo_moment_match_cov", ("loo_moment_match",),
     "loo_moment_match_cov needs loo_moment_match: it is the covariance step of the matching of its cells"),
    ("exact_loo_moment_match_cov", ("exact_loo_moment_match",),
     "exact_loo_moment_match_cov needs exact_loo_moment_match: it is the covariance step of the matching of its cells"),
    ("approximation_loo_moment_match", ("check_approximation_loo",),
     "approximation_loo_moment_match needs check_approximation_loo: it matches the moments of the cells whose k-hat its PSIS-LOO "
     "finds too high"),
    ("exact_approximation_loo_moment_match", ("exact_approximation_loo_intervals",),
     "exact_approximation_loo_moment_match needs exact_approximation_loo_intervals: it matches the moments of the cells whose "
     "k-hat their PSIS finds too high"),
)
LOO_MOMENT_MATCH_MCSE = ("loo_mcse cannot be combined with loo_moment_match: the Monte-Carlo standard error and n_eff are those of "
                         "plain PSIS weights and are not given for a matched cell")

CHECK_OPTIONS = tuple(c.keyword for c in CHECKS) + tuple(m[0] for m in MODIFIERS)


def select_checks(options, approximate_posterior_inference, over_ranks=False):
    """Refuses what a pass of this kind cannot report (ValueError, the option's name first) and returns the options that are
    set, {keyword: value}: what travels from identify_outliers to the pass and on to read_checks. `options` maps every keyword
    of CHECK_OPTIONS to its value (the caller's locals() will do)."""
    kind = "advi" if approximate_posterior_inference else "nuts"
    for chk in sorted(CHECKS, key=lambda c: c.order):
        if options[chk.keyword]:
            if chk.kind not in (None, kind):
                raise ValueError(chk.refusal)
            if over_ranks and not chk.ranks:
                raise ValueError(f"{chk.keyword} is not available for passes over several ranks")
    r_eff = options["loo_r_eff"]
    if r_eff is not None and not (isinstance(r_eff, str) and r_eff == "auto"):
        raise ValueError(f'loo_r_eff must be None or "auto", not {r_eff!r}')
    for keyword, needs, refusal in MODIFIERS:
        if options[keyword] and not any(options[k] for k in needs):
            raise ValueError(refusal)
    if options["loo_mcse"] and options["loo_moment_match"]:
        raise ValueError(LOO_MOMENT_MATCH_MCSE)
    return {k: options[k] for k in CHECK_OPTIONS if options[k]}


def read_checks(fit, ctx, selected, res):
    """Runs the selected diagnostics' readers on `fit` in the order of CHECKS, fills their fields of `res` and returns their
    warning messages."""
    msgs = []
    for chk in CHECKS:
        if selected.get(chk.keyword) and not (chk.cells and ctx.pooled and ctx.K == 0):
            result = chk.read(fit, ctx)
            setattr(res, chk.field, result)
            if chk.warn is not None:
                msgs += chk.warn(result, fit)
    return msgs


def do_inference(counts, X, exposure_rate, how_many_to_check, *,
                 approximate_posterior_inference=False,
                 approximate_posterior_analysis=False,
                 lambda_mu_mu=5.612671,
                 cores=4,
                 adj_prob_theshold=0.05,
                 how_many_posterior_draws=1000,
                 to_exclude=None,
                 truncation_compensation=1.0,
                 save_generated_quantities=False,
                 pass_fit=False,
                 seed=1,
                 device=0,
                 model=None,
                 chains=None,
                 devices=None,
                 launch=None,
                 check_convergence=False,
                 check_approximation=False,
                 check_loo=False,
                 check_loo_intervals=False,
                 loo_r_eff=None,
                 loo_mcse=False,
                 loo_moment_match=False,
                 check_approximation_loo=False,
                 check_approximation_loo_intervals=False,
                 exact_intervals=False,
                 exact_loo_intervals=False,
                 exact_approximation_loo_intervals=False,
                 exact_loo_moment_match=False,
                 loo_moment_match_split=False,
                 exact_loo_moment_match_split=False,
                 loo_moment_match_cov=False,
                 exact_loo_moment_match_cov=False,
                 approximation_loo_moment_match=False,
                 exact_approximation_loo_moment_match=False,
                 per_sample="lds"):
    """One inference pass (discovery or test) of ppcseq on the GPU.

    counts            G x S integer matrix, genes ordered with the `how_many_to_check` checked genes first
                      (R/utilities.R:949-952) and samples in S order (:955-958)
    X                 S x C design matrix (R/utilities.R:887-900)
    exposure_rate     length S, `-log(multiplier)` (R/methods.R:236)
    to_exclude        iterable of (S, G) 1-based pairs as in the reference's tibble (R/methods.R:292-300),
                      or an int array of 0-based cell ids g*S+s
    devices           several HIP devices of this process: the chains are split over them (the reference runs its chains in
                      `cores` worker processes, R/utilities.R:1500-1501) and the credible intervals come from the POOLED
                      draws, as rstan::summary does over merged chains (:685-703). One process per GPU under
                      torch.distributed: ppcseq_amd.distributed.do_inference.
    launch            (lanes_per_gene, workgroups) pins the log-likelihood launch (0 = automatic); by default it follows the number of
                      chains per launch, and results agree to rounding, not bit for bit, between geometries
    check_convergence the checks rstan::sampling runs after a NUTS fit: R-hat and bulk / tail ESS of alpha_sub_1 and lp__ (the
                      parameters the reference saves besides counts_rng) on the device (Fit.summary), kept as
                      `res.convergence` and reported as RuntimeWarning (convergence_warnings). devices=[...]: over the pooled
                      chains, alpha_sub_1 only (the pooled fit holds no lp__). Not for an ADVI pass.
    check_approximation what rstan::vb reports after an ADVI fit: the Pareto k diagnostic (PSIS) of the log ratios log_p - log_g
                      of the output draws and the per-parameter k-hat of alpha_sub_1, on the device (Fit.psis), kept as
                      `res.approximation` (the overall k-hat last, column -1) and reported as RuntimeWarning from the
                      overall k-hat (approximation_warnings). Not for a NUTS pass.
    check_loo         what rstan::loo(fit) reports next: PSIS-LOO of every checked cell (elpd_loo, p_loo, looic, khat; loo's
                      estimates over the cells not excluded) on the device (Fit.loo), kept as `res.loo` and reported as
                      RuntimeWarning when a k-hat is too high (loo_warnings). An excluded cell holds its exact held-out
                      density. devices=[...]: over the pooled chains. Not for an ADVI pass.
    check_loo_intervals  the leave-one-out predictive interval and LOO-PIT of every checked cell from this pass's own fit
                      (loo::E_loo / bayesplot::ppc_loo_intervals, ppc_loo_pit) on the device (Fit.loo_predict), at the pass's
                      interval probabilities, seed and truncation compensation, kept as `res.loo_intervals`. It raises no
                      warning (the k-hat warnings are check_loo's) and changes no flag. devices=[...]: over the pooled chains.
                      Not for an ADVI pass.
    loo_r_eff         None: check_loo, check_loo_intervals and exact_loo_intervals take r_eff = 1 (loo::loo(log_lik)). "auto": the
                      relative efficiency of every checked cell from the fit's own chains on the device (Fit.relative_eff; 1
                      where it is not defined), as rstan::loo(fit) does; the results then carry it as `r_eff`. devices=[...]:
                      over the pooled chains (the split is the same). Needs check_loo, check_loo_intervals or
                      exact_loo_intervals.
    loo_mcse          True: `res.loo` also carries loo's pointwise `mcse_elpd_loo` and `n_eff` of every checked cell and
                      `mcse_elpd_loo_total` (Fit.loo(mcse=True); pareto_k_table reads it). It raises no further warning.
                      devices=[...]: over the pooled chains. Needs check_loo.
    loo_moment_match  True: `res.loo` comes from Fit.loo_moment_match: the cells whose k-hat exceeds loo_threshold get gene-local
                      moment matching (a restatement of loo::loo_moment_match on the cell's own gene; its split and
                      covariance steps are loo_moment_match_split and loo_moment_match_cov); `res.loo` then also carries `khat_before`, `iterations`, `scale`, `shift` and
                      `k_threshold`, and the k-hat warning reads the final `khat`. Flags and frame are those of the call
                      without it. devices=[...]: over the pooled chains (no lp__ is needed). Needs check_loo; not with loo_mcse
                      (a matched cell has no mcse / n_eff).
    check_approximation_loo  check_loo for an ADVI pass: PSIS-LOO of every checked cell with the correction for the approximation
                      (loo::loo_approximate_posterior; ratios (log_p - log_g) - log_lik, r_eff = 1) on the device
                      (Fit.loo_approximate_posterior), kept as `res.approximation_loo` and reported as RuntimeWarning when a k-hat
                      is too high (loo_warnings). No mcse / n_eff. Not for a NUTS pass.
    check_approximation_loo_intervals  check_loo_intervals for an ADVI pass, under the same weights
                      (Fit.loo_predict_approximate_posterior) at the pass's interval probabilities, seed and truncation
                      compensation, kept as `res.approximation_loo_intervals`. No warning, no flag changes. Not for a NUTS pass.
    exact_intervals   the exact posterior-predictive tail probabilities and interval of every checked cell (Fit.ppc_exact: the
                      average over the kept draws of negative-binomial cdfs, nothing sampled) at the pass's interval
                      probabilities and truncation compensation, kept as `res.exact_intervals`. NUTS and ADVI passes;
                      devices=[...]: over the pooled chains. Reported, not acted on: the flags stay those of the sampled intervals.
    exact_loo_intervals  the exact leave-one-out predictive tail probabilities and interval of every checked cell
                      (Fit.loo_predict_exact: the average of the draws' negative-binomial cdfs under check_loo_intervals' PSIS
                      weights, nothing sampled; khat and the two ends of the LOO-PIT beside them) at the pass's interval
                      probabilities and truncation compensation, kept as `res.exact_loo_intervals`. It raises no warning (the
                      k-hat warnings are check_loo's) and changes no flag. devices=[...]: over the pooled chains. Not for an ADVI
                      pass.
    exact_approximation_loo_intervals  exact_loo_intervals for an ADVI pass, under the weights of check_approximation_loo
                      (Fit.loo_predict_exact_approximate_posterior), kept as `res.exact_approximation_loo_intervals`. No
                      warning, no flag changes. Not for a NUTS pass.
    exact_loo_moment_match  True: `res.exact_loo_intervals` comes from Fit.loo_predict_exact_moment_match: the cells whose k-hat
                      exceeds loo_threshold -- the outliers the check exists to find -- are matched as loo_moment_match matches
                      them and their interval and tail probabilities are taken under the matched weights at the matched draws;
                      the result then also carries `khat_before`, `iterations`, `scale`, `shift` and `k_threshold`, and `khat` is
                      the final one. Flags and frame are those of the call without it. devices=[...]: over the pooled chains.
                      Needs exact_loo_intervals. loo_moment_match itself affects `res.loo` only.
    loo_moment_match_split  True: loo_moment_match reads Fit.loo_moment_match(split=True): the split transformation of
                      loo::loo_moment_match on the matched cells (the first half of the draws in the fit's order is transformed,
                      the rest kept, all weighted against the mixture they come from); `res.loo` then also carries
                      `elpd_loo_matched` and `khat_split`, and the k-hat warning keeps reading `khat`, the matching's final one.
                      Needs loo_moment_match.
    exact_loo_moment_match_split  True: exact_loo_moment_match reads Fit.loo_predict_exact_moment_match(split=True), the same
                      transformation for the predictive; `res.exact_loo_intervals` then also carries `khat_split`. Needs
                      exact_loo_moment_match.
    loo_moment_match_cov  True: loo_moment_match reads Fit.loo_moment_match(cov=True): the covariance step as a third candidate of
                      the matching (restated from the paper and the published package; not run against R); `res.loo` then carries
                      `transform` in place of `scale`, and `cov_iterations`. Free to combine with loo_moment_match_split; refused
                      with loo_mcse as loo_moment_match is. Needs loo_moment_match. It affects `res.loo` only.
    exact_loo_moment_match_cov  True: exact_loo_moment_match reads Fit.loo_predict_exact_moment_match_cov, the predictive under the
                      weights of the matching with the covariance step at the affinely matched draws;
                      `res.exact_loo_intervals` then carries `transform` in place of `scale`, and `cov_iterations`. Free to
                      combine with exact_loo_moment_match_split. devices=[...]: over the pooled chains. Needs
                      exact_loo_moment_match.
    approximation_loo_moment_match  True: `res.approximation_loo` comes from Fit.loo_moment_match_approximate_posterior: the cells
                      whose k-hat exceeds loo_threshold get the gene-local moment matching of loo_moment_match under the weights
                      of the approximation (no split transformation, no covariance step: a matched k-hat is necessary, not
                      sufficient, and says nothing of a mismatch in the hyper-parameters, which an overall k-hat that is itself
                      too high reports); the result then also carries
                      `khat_before`, `iterations`, `scale`, `shift` and `k_threshold`, and the k-hat warning reads the final
                      `khat`. Flags and frame are those of the call without it. Needs check_approximation_loo.
    exact_approximation_loo_moment_match  True: `res.exact_approximation_loo_intervals` comes from
                      Fit.loo_predict_exact_moment_match_approximate_posterior: the interval and tail probabilities of those
                      cells are taken under the matched weights at the matched draws; the result carries the same further keys.
                      Flags and frame are those of the call without it. Needs exact_approximation_loo_intervals.
    per_sample        "lds" | "stream" | "auto": where the log-likelihood kernel keeps the per-sample constants, for every model
                      this pass creates (_lib.Model). "lds" refuses a design whose S * C doubles do not fit LDS beside the
                      tables (S <= 8 704 at two columns, 1 088 at sixteen); "auto" streams them from global memory there.
    Returns an InferenceResult.
    """
    if per_sample not in _lib.PER_SAMPLE:
        raise ValueError('per_sample must be "lds", "stream" or "auto"')
    counts = np.asarray(counts)
    if counts.ndim != 2:
        # R/utilities.R:1360-1361
        raise ValueError("The input data frame does not represent a rectangular structure. "
                         "Each transcript must be present in all samples.")
    if not np.issubdtype(counts.dtype, np.integer):
        raise TypeError("The abundance column must be of class integer")   # R/methods.R:146-153
    G, S = counts.shape
    K = int(how_many_to_check)
    X = np.asarray(X, dtype=np.float64).reshape(S, -1)

    chains, n_iter, warmup = pass_plan(how_many_posterior_draws, approximate_posterior_analysis, chains, cores)
    excl = _to_cell_ids(to_exclude, S)
    checks = select_checks(locals(), approximate_posterior_inference)
    if devices is not None and len(devices) > 1 and (save_generated_quantities or pass_fit or model is not None or approximate_posterior_inference):
        raise ValueError("devices=[...] splits the chains of a NUTS fit over several devices and pools their draws: it cannot "
                         "be combined with save_generated_quantities, pass_fit, a caller's model or approximate_posterior_inference")
    if devices is not None and len(devices) > 1 and not approximate_posterior_inference:
        return _do_inference_devices(counts, X, exposure_rate, K, list(devices), chains, n_iter, warmup, excl,
                                     lambda_mu_mu, approximate_posterior_analysis, adj_prob_theshold,
                                     how_many_posterior_draws, truncation_compensation, seed, launch, checks, per_sample)
    if devices is not None and len(devices) >= 1 and model is None:
        device = devices[0]
    own_model = model is None
    if own_model:
        model = _lib.Model(counts, X, exposure_rate, K, lambda_mu_mu=lambda_mu_mu, excl=excl, device=device, **_route(per_sample))
    else:
        model.set_exclusions(excl)
    if launch is not None:
        model.set_launch(*launch)
    if approximate_posterior_inference:
        # vb_iterative(model, output_samples = draws_practical, iter = 50000, tol_rel_obj = 0.005)
        # (R/utilities.R:1487-1494; the reference passes no seed to vb -- here the run is seeded and reproducible)
        # vb_iterative retries a failed vb() call (R/utilities.R:246-278): here bounded, attempt k with seed + k
        output_samples = 1000 if approximate_posterior_analysis else how_many_posterior_draws      # R/utilities.R:1372
        fit = model.fit_advi(output_samples=int(output_samples), iter=50000, tol_rel_obj=0.005, seed=seed, max_attempts=5)
    else:
        fit = model.fit_nuts(chains=chains, iter=n_iter, warmup=warmup, seed=seed)
    try:
        p = float(adj_prob_theshold)
        if approximate_posterior_analysis:
            # R/utilities.R:733-784: resample the posterior, rnbinom per cell
            out = fit.ppc(truncation_compensation, p, 1 - p, seed=seed, n_gen=int(how_many_posterior_draws),
                          resample=True, return_counts_rng=False)
            ci, rng = out, None
        else:
            out = fit.ppc(truncation_compensation, p, 1 - p, seed=seed, n_gen=0, resample=False,
                          return_counts_rng=bool(save_generated_quantities))
            ci, rng = out if save_generated_quantities else (out, None)
        # slope = posterior mean of alpha_sub_1 (R/utilities.R:1531, :1250-1263)
        slope = fit.columns(_alpha_sub_1(fit, K)).reshape(-1, K).mean(axis=0) if K else np.zeros(0)
        res = _post_process(counts[:K], ci, slope, X)
        res.total_draws = S * K * int(how_many_posterior_draws)   # R/utilities.R:1544
        res.chains, res.iter = chains, n_iter
        res.diagnostics = fit.advi_info() if approximate_posterior_inference else fit.diagnostics()
        msgs = [] if approximate_posterior_inference else hmc_warnings(res.diagnostics, warmup)
        msgs += read_checks(fit, CheckContext(K, p, seed, truncation_compensation, checks.get("loo_r_eff"),
                                              checks.get("loo_mcse", False),
                                              loo_moment_match=bool(checks.get("loo_moment_match", False)),
                                              exact_loo_moment_match=bool(checks.get("exact_loo_moment_match", False)),
                                              loo_moment_match_split=bool(checks.get("loo_moment_match_split", False)),
                                              exact_loo_moment_match_split=bool(checks.get("exact_loo_moment_match_split", False)),
                                              loo_moment_match_cov=bool(checks.get("loo_moment_match_cov", False)),
                                              exact_loo_moment_match_cov=bool(checks.get("exact_loo_moment_match_cov", False)),
                                              approximation_loo_moment_match=bool(checks.get("approximation_loo_moment_match", False)),
                                              exact_approximation_loo_moment_match=bool(
                                                  checks.get("exact_approximation_loo_moment_match", False))),
                                  checks, res)
        for msg in msgs:
            warnings.warn(msg, RuntimeWarning, stacklevel=2)
        res.counts_rng = rng
        if pass_fit:
            res.fit = fit
    finally:
        if not pass_fit:
            fit.close()
            if own_model:
                model.close()
    return res


def _to_cell_ids(to_exclude, S):
    if to_exclude is None:
        return np.zeros(0, np.int32)
    a = np.asarray(to_exclude)
    if a.size == 0:
        return np.zeros(0, np.int32)
    if a.ndim == 2 and a.shape[1] == 2:          # (S, G) pairs, 1-based
        return ((a[:, 1].astype(np.int64) - 1) * S + (a[:, 0].astype(np.int64) - 1)).astype(np.int32)
    return a.astype(np.int32).ravel()


def _post_process(counts_checked, ci, slope, X):
    """check_if_within_posterior (R/utilities.R:651-663) + add_deleterious_if_covariate_exists (:493-513)."""
    K, S = counts_checked.shape
    mean, sd, lower, upper = ci[..., 0], ci[..., 1], ci[..., 2], ci[..., 3]
    y = counts_checked.astype(np.float64)
    ppc = (y >= lower) & (y <= upper)                       # dplyr::between is inclusive
    higher = (~ppc) & (y > mean)
    is_group_high = delet = None
    if X.shape[1] > 1:
        f = X[:, 1]
        right = f > f.mean()
        is_group_high = ((slope[:, None] > 0) & right[None, :]) | ((slope[:, None] < 0) & ~right[None, :])
        delet = (~ppc) & (higher == is_group_high)
    return InferenceResult(K=K, S=S, mean=mean, sd=sd, lower=lower, upper=upper, ppc=ppc,
                           is_higher_than_mean=higher, slope=slope, is_group_high=is_group_high,
                           deleterious_outliers=delet, total_draws=0, chains=0, iter=0)


def checked_columns(G, C, K):
    """Columns of the unconstrained vector that belong to the K checked genes and the hyper-parameters, in the order of
    the unconstrained vector of a model that holds ONLY those K genes (Stan declaration order, .stan:183-197)."""
    n2 = max(C - 2, 0)
    off_a1, off_a2 = 3 + G, 3 + G + K
    off_sr = off_a2 + n2 * K
    return np.concatenate([np.arange(3), 3 + np.arange(K), off_a1 + np.arange(K), off_a2 + np.arange(n2 * K),
                           off_sr + np.arange(K), off_sr + G + np.arange(3)]).astype(np.int32)


def _route(per_sample):
    """The keyword of _lib.Model for a pass's per_sample: nothing for the default, so that a default pass creates its models exactly
    as before the keyword existed"""
    return {} if per_sample == "lds" else {"per_sample": per_sample}


def pooled_summary(counts, X, exposure_rate, K, draws_checked, *, lambda_mu_mu, approximate_posterior_analysis,
                   adj_prob_theshold, how_many_posterior_draws, truncation_compensation, seed, device=0, excl=None, checks=None,
                   per_sample="lds"):
    """Credible intervals, slopes and flags from the pooled draws of all chains (rstan::summary over merged chains,
    R/utilities.R:685-703): `draws_checked` is [chains, n_keep, len(checked_columns)] in global chain order. The
    posterior-predictive kernel runs on a model that holds the K checked genes only -- cell ids g*S+s and draw indices are
    those of the full model, so the result is what a single fit of all the chains gives, bit for bit. `checks`: the diagnostics
    to read over the pooled chains as well, as select_checks returns them (do_inference says what each reports; their warnings
    are raised here, on the caller). For those that read the checked genes' cells the small model carries those cells of `excl`
    (0-based cell ids of the full model), so that the cells excluded from the fit are held out or reported as excluded."""
    counts = np.asarray(counts)
    X = np.asarray(X, dtype=np.float64).reshape(counts.shape[1], -1)
    checks = checks or {}
    for chk in CHECKS:
        if checks.get(chk.keyword) and not chk.pooled:
            raise ValueError(f"{chk.keyword} is not available over pooled chains")
    small_excl = None
    if excl is not None and any(chk.cells for chk in CHECKS if checks.get(chk.keyword)):
        e = np.asarray(excl, dtype=np.int64).ravel()
        small_excl = e[e < K * counts.shape[1]].astype(np.int32)
    small = _lib.Model(counts[:K], X, exposure_rate, K, lambda_mu_mu=lambda_mu_mu, device=device, excl=small_excl, **_route(per_sample))
    try:
        fit = small.fit_from_draws(draws_checked)
        try:
            p = float(adj_prob_theshold)
            if approximate_posterior_analysis:
                ci = fit.ppc(truncation_compensation, p, 1 - p, seed=seed, n_gen=int(how_many_posterior_draws), resample=True)
            else:
                ci = fit.ppc(truncation_compensation, p, 1 - p, seed=seed, n_gen=0, resample=False)
            slope = fit.columns(_alpha_sub_1(fit, K)).reshape(-1, K).mean(axis=0) if K else np.zeros(0)
            res = _post_process(counts[:K], ci, slope, X)
            res.total_draws = counts.shape[1] * K * int(how_many_posterior_draws)
            msgs = read_checks(fit, CheckContext(K, p, seed, truncation_compensation, checks.get("loo_r_eff"),
                                                 checks.get("loo_mcse", False), pooled=True,
                                                 loo_moment_match=bool(checks.get("loo_moment_match", False)),
                                              exact_loo_moment_match=bool(checks.get("exact_loo_moment_match", False)),
                                              loo_moment_match_split=bool(checks.get("loo_moment_match_split", False)),
                                              exact_loo_moment_match_split=bool(checks.get("exact_loo_moment_match_split", False)),
                                              loo_moment_match_cov=bool(checks.get("loo_moment_match_cov", False)),
                                              exact_loo_moment_match_cov=bool(checks.get("exact_loo_moment_match_cov", False)),
                                              approximation_loo_moment_match=bool(checks.get("approximation_loo_moment_match", False)),
                                              exact_approximation_loo_moment_match=bool(
                                                  checks.get("exact_approximation_loo_moment_match", False))),
                                  checks, res)
        finally:
            fit.close()
    finally:
        small.close()
    for msg in msgs:
        warnings.warn(msg, RuntimeWarning, stacklevel=2)
    return res


def fit_chain_block(counts, X, exposure_rate, K, cols, *, device, chains, n_iter, warmup, seed, chain_id_offset, lambda_mu_mu,
                    excl, launch, per_sample="lds"):
    """One device's share of a pass whose chains are dealt out (to the devices of this process, or to the ranks of a job): fits
    `chains` chains with the global ids chain_id_offset, ... on `device` and returns their columns `cols`,
    [chains, n_keep, len(cols)]."""
    m = _lib.Model(counts, X, exposure_rate, K, lambda_mu_mu=lambda_mu_mu, excl=excl, device=device, **_route(per_sample))
    try:
        if launch is not None:
            m.set_launch(*launch)
        f = m.fit_nuts(chains=chains, iter=n_iter, warmup=warmup, seed=seed, chain_id_offset=chain_id_offset)
        try:
            return f.columns(cols)
        finally:
            f.close()
    finally:
        m.close()


def _do_inference_devices(counts, X, exposure_rate, K, devices, chains, n_iter, warmup, excl, lambda_mu_mu,
                          approximate_posterior_analysis, adj_prob_theshold, how_many_posterior_draws,
                          truncation_compensation, seed, launch, checks, per_sample="lds"):
    """Chains split over several devices of this process (one host thread per device; the C ABI allows different handles
    on different threads), pooled summary on the first device."""
    import threading
    nd = min(len(devices), chains)
    per = int(math.ceil(chains / nd))
    cols = checked_columns(counts.shape[0], X.shape[1], K)
    parts, errs = [None] * nd, [None] * nd

    def work(r):
        n = min(per, chains - r * per)
        if n <= 0:
            return
        try:
            parts[r] = fit_chain_block(counts, X, exposure_rate, K, cols, device=devices[r], chains=n, n_iter=n_iter,
                                       warmup=warmup, seed=seed, chain_id_offset=r * per, lambda_mu_mu=lambda_mu_mu,
                                       excl=excl, launch=launch, per_sample=per_sample)
        except Exception as e:          # re-raised on the calling thread
            errs[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(nd)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for e in errs:
        if e is not None:
            raise e
    pooled = np.concatenate([p for p in parts if p is not None], axis=0)
    res = pooled_summary(counts, X, exposure_rate, K, pooled, lambda_mu_mu=lambda_mu_mu,
                         approximate_posterior_analysis=approximate_posterior_analysis, adj_prob_theshold=adj_prob_theshold,
                         how_many_posterior_draws=how_many_posterior_draws, truncation_compensation=truncation_compensation,
                         seed=seed, device=devices[0], excl=excl, checks=checks, per_sample=per_sample)
    res.chains, res.iter = chains, n_iter
    return res
