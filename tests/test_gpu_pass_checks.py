"""The optional diagnostics of a pass do not touch each other: do_inference with all of them on reports, bit for bit, what it
reports with each of them alone -- every array of every result dict, the intervals and the flags. They share one table and one
reader (inference.CHECKS, read_checks); each read is a pure function of the fit, and this pins that sharing has not coupled them.
A synthetic 8 x 6 model with 2 checked genes (`~ 1 + x`, x binary), one seed, one launch geometry."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NUTS = dict(check_convergence={}, check_loo=dict(loo_r_eff="auto", loo_mcse=True), check_loo_intervals=dict(loo_r_eff="auto"),
            exact_intervals={})                       # option -> the modifiers it takes when all are on
ADVI = dict(check_approximation={}, check_approximation_loo={}, check_approximation_loo_intervals={}, exact_intervals={})
FIELD = dict(check_convergence="convergence", check_loo="loo", check_loo_intervals="loo_intervals", exact_intervals="exact_intervals",
             check_approximation="approximation", check_approximation_loo="approximation_loo",
             check_approximation_loo_intervals="approximation_loo_intervals")
PLAIN = ("mean", "sd", "lower", "upper", "ppc", "is_higher_than_mean", "slope", "is_group_high", "deleterious_outliers")


def same(a, b, where):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), where


def together_and_alone(options, **how):
    from ppcseq_amd.inference import do_inference
    from ppcseq_amd.synth import synth
    d = synth(8, 6, K=2, seed=4)
    run = lambda **kw: do_inference(d["counts"], d["X"], d["exposure"], 2, how_many_posterior_draws=300, cores=3, seed=23,  # noqa: E731
                                    launch=(8, 0), **how, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        both = {}
        for option, modifiers in options.items():
            both.update({option: True}, **modifiers)
        full = run(**both)
        for option, modifiers in options.items():
            alone = run(**{option: True}, **modifiers)
            for other in options:
                assert (getattr(alone, FIELD[other]) is not None) == (other == option), (option, other)
            assert getattr(full, FIELD[option]) is not None, option
            same(getattr(full, FIELD[option]), getattr(alone, FIELD[option]), f"{how} {option}")
            for k in PLAIN:
                same(getattr(full, k), getattr(alone, k), f"{how} {option}: {k}")
            assert (full.chains, full.iter, full.total_draws) == (alone.chains, alone.iter, alone.total_draws)


def test_nuts_options_together_and_alone():
    together_and_alone(NUTS)


def test_advi_options_together_and_alone():
    together_and_alone(ADVI, approximate_posterior_inference=True)


def test_pooled_nuts_options_together_and_alone():
    together_and_alone(NUTS, devices=[0, 0])
