"""The cells of the exact predictive under the weights of the matching with the covariance step, shared by
tests/test_loo_mm_cov_exact_host.py (CPU) and tests/test_gpu_loo_mm_cov_exact.py (device): the checked-gene cells of
tests/loo_mm_cov_cases.designed() and designed(widest=True), at their own thresholds, r_eff and max_iters. A predictive entry
serves checked genes only: the cells of the unchecked genes of those lists are UNCHECKED, which the device test uses for the
refusal."""
from tests import loo_mm_cov_cases as cov_cases

gene_of = cov_cases.gene_of
draw_set = cov_cases.draw_set


def _checked(c):
    return bool(gene_of(c)["checked"])


ALL = cov_cases.designed() + cov_cases.designed(widest=True)
CELLS = [c for c in ALL if _checked(c)]
UNCHECKED = [c for c in ALL if not _checked(c)]


def kw(c):
    return dict(r_eff=c["r_eff"], k_threshold=c["k_threshold"], max_iters=c["max_iters"])
