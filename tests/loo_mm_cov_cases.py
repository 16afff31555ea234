"""The designed cells of gene-local moment matching with the covariance step, shared by tests/test_loo_mm_cov_host.py (CPU) and
tests/test_gpu_loo_mm_cov.py (device). They reuse the committed draw sets: tests/loo_mm_cases.py's tiny model (C = 2) and
tests/wide_design_cases.py's "covariate" (C = 3) and "factor4" (C = 4). `kinds` are the accepted candidates under the restatement
(tests/loo_mm_cov_restate.point), which tests/test_loo_mm_cov_host.py qualifies first (ten perturbations of every ratio by 1e-9
relative leave them unchanged). Every kind listed below qualifies; none had to be left out."""
from tests import loo_mm_cases as cases
from tests import wide_design_cases as wide

WIDE = ("covariate", "factor4", "long")
FACTOR4 = dict(set="factor4", g=0, s=5)              # "factor4: khat stays above the threshold" of wide_design_cases.designed()


def draw_set(name):
    return wide.draw_set(name) if name in WIDE else cases.draw_set(name)


def gene_of(c):
    return cases.gene_of(draw_set(c["set"]), c["g"])


def designed():
    """dicts of name, set, g, s, r_eff, k_threshold, max_iters and `kinds`, as tests/loo_mm_cases.designed() gives them"""
    cs = []

    def add(name, set_, g, s, kinds, r_eff=1.0, k_threshold=0.7, max_iters=30):
        cs.append(dict(name=name, set=set_, g=g, s=s, kinds=kinds, r_eff=r_eff, k_threshold=k_threshold, max_iters=max_iters))

    add("factor4: kind 3 accepted, khat ends below 0.7 (d = 5)", "factor4", 0, 5, [1, 3, 1])
    add("d = 3", "b", 0, 3, [1, 3], k_threshold=0.5)
    add("d = 2 of the unchecked gene inside C = 3; 3 is the first accepted kind", "covariate", 2, 3, [3], k_threshold=0.1)
    add("two covariance steps and a scale step after one", "factor4", 0, 5, [1, 3, 1, 3, 2], k_threshold=0.5)
    add("five shifts, then 3 (gene 1 of factor4)", "factor4", 1, 2, [1, 1, 1, 1, 1, 3], k_threshold=0.5)
    add("nine steps with a 3 and a 2 among them (d = 4)", "covariate", 0, 5, [1, 1, 1, 1, 3, 1, 1, 2, 1], k_threshold=0.3)
    add("3 tried and refused at once: the loop ends", "b", 0, 0, [], k_threshold=0.2)
    add("3 tried and refused after a shift: the loop ends", "factor4", 0, 5, [1], r_eff=0.4)
    add("stopped by max_iters right after a kind 3", "factor4", 0, 5, [1, 3], max_iters=2)
    add("r_eff = 0.5", "b", 0, 3, [1, 3, 2], r_eff=0.5, k_threshold=0.3)
    add("densities that are not finite at some draws", "c, planted", 0, 3, [2, 1, 1, 1, 1, 1, 1, 2, 1, 3], k_threshold=0.3)
    add("excluded cell", "factor4", 1, 3, [])
    add("nan cell", "nan", 1, 1, [])
    add("max_iters = 0", "factor4", 0, 5, [], max_iters=0)
    return cs
