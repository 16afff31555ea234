"""The designed cells of gene-local moment matching with the covariance step, shared by tests/test_loo_mm_cov_host.py (CPU) and
tests/test_gpu_loo_mm_cov.py (device). They reuse the committed draw sets: tests/loo_mm_cases.py's tiny model (C = 2) and
tests/wide_design_cases.py's "covariate" (C = 3) and "factor4" (C = 4). `kinds` are the accepted candidates under the restatement
(tests/loo_mm_cov_restate.point), which tests/test_loo_mm_cov_host.py qualifies first (ten perturbations of every ratio by 1e-9
relative leave them unchanged). Every kind listed below qualifies; none had to be left out. designed(widest=True): the cells of
the widest designs ("columns8", "columns16", "columns15"), which tests/test_widest_designs_host.py qualifies and
tests/test_gpu_widest_designs.py runs on the device."""
from tests import loo_mm_cases as cases
from tests import wide_design_cases as wide

WIDE = ("covariate", "factor4", "long", "columns8", "columns16", "columns15")
# The draw counts of the covariance kernel at the widest designs (prefixes of the sets; split=True): the wavefront, the workgroup's
# stride, and n <= d = C + 1, d + 1. `cells`: one cell of a checked gene and the unchecked gene's outlier, which qualify at every
# count (tests/test_widest_designs_host.py asserts it) and are the two that tests/test_gpu_widest_designs.py holds to the CPU build.
WIDEST_COUNTS = dict(columns16=dict(ns=(16, 17, 18, 63, 64, 65, 255, 256, 257), threshold=0.3, cells=((1, 4), (2, 1))),
                     columns8=dict(ns=(8, 9, 10, 64, 257), threshold=0.3, cells=((0, 6), (2, 1))))
FACTOR4 = dict(set="factor4", g=0, s=5)              # "factor4: khat stays above the threshold" of wide_design_cases.designed()


def draw_set(name):
    return wide.draw_set(name) if name in WIDE else cases.draw_set(name)


def gene_of(c):
    return cases.gene_of(draw_set(c["set"]), c["g"])


def designed(widest=False):
    """dicts of name, set, g, s, r_eff, k_threshold, max_iters and `kinds`, as tests/loo_mm_cases.designed() gives them.
    widest: the cells of wide_design_cases' "columns8" (d = 9), "columns16" (d = 17) and "columns15" (d = 16) instead, a list of
    their own (tests/test_widest_designs_host.py, tests/test_gpu_widest_designs.py). The unchecked gene's cells but its outlier
    start at a khat of 0.2 or less, so its covariance steps are reached at thresholds at and below 0.05."""
    cs = []

    def add(name, set_, g, s, kinds, r_eff=1.0, k_threshold=0.7, max_iters=30):
        cs.append(dict(name=name, set=set_, g=g, s=s, kinds=kinds, r_eff=r_eff, k_threshold=k_threshold, max_iters=max_iters))

    if widest:
        add("d = 17: shift, then 3 at the outlier", "columns16", 0, 5, [1, 3], k_threshold=0.5)
        add("d = 17: a scale on the full matrix after a 3", "columns16", 0, 7, [1, 3, 2], k_threshold=0.3)
        add("d = 17: gene 1, a scale after a 3", "columns16", 1, 4, [1, 3, 2], k_threshold=0.5)
        add("d = 17: 3 after a scale, two scales after it", "columns16", 0, 8, [2, 3, 2, 2], k_threshold=0.3)
        add("d = 17: ten steps, three of them 3, two of those after one another", "columns16", 0, 8, [2, 3, 2, 2, 1, 2, 1, 2, 3, 3],
            k_threshold=0.1)
        add("d = 17: gene 1, shift and scale after a 3", "columns16", 1, 13, [1, 3, 1, 2], k_threshold=0.3)
        add("d = 17: stopped by max_iters right after a 3", "columns16", 0, 5, [1, 3], k_threshold=0.3, max_iters=2)
        add("d = 2 inside nc = 17: 3 in the unchecked gene, rows 0 and 16", "columns16", 2, 17, [2, 3, 2], k_threshold=-0.3)
        add("d = 2 inside nc = 17: r_eff = 0.5", "columns16", 2, 19, [2, 3], r_eff=0.5, k_threshold=-0.1)
        add("d = 17: 3 tried and refused after a shift: the loop ends", "columns16", 0, 10, [1], k_threshold=0.1)
        add("d = 17: excluded cell", "columns16", 1, 3, [])
        add("d = 9: two shifts, then 3", "columns8", 0, 5, [1, 1, 3])
        add("d = 9: 3 between shifts", "columns8", 0, 6, [1, 3, 1], k_threshold=0.5)
        add("d = 9: gene 1, a scale after a 3", "columns8", 1, 5, [1, 2, 3, 1, 2], k_threshold=0.5)
        add("d = 9: three 3s, a scale between them", "columns8", 0, 4, [1, 2, 3, 2, 3, 3], k_threshold=0.3)
        add("d = 9: 3 is the first accepted kind", "columns8", 1, 7, [3], k_threshold=0.3)
        add("d = 2 inside nc = 9: 3 in the unchecked gene", "columns8", 2, 0, [1, 3], k_threshold=0.05)
        add("d = 9: 3 tried and refused after two steps: the loop ends", "columns8", 1, 4, [1, 2], k_threshold=0.1)
        add("d = 16: two shifts, then 3 ((C + 1)^2 = 256)", "columns15", 0, 13, [1, 1, 3], k_threshold=0.5)
        add("d = 16: gene 1, shift, then 3", "columns15", 1, 10, [1, 3], k_threshold=0.5)
        return cs
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
