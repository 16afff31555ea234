"""The ADVI cases shared by tests/test_advi_restate.py (CPU) and tests/test_gpu_advi.py (device), and their qualification: a case
is only compared across implementations if rounding cannot move its decisions (DESIGN.md "ADVI").

A case's yardstick Y is how far gradient errors of the size the suite allows the device (1e-10 (1 + |g|), the tolerance of
test_log_prob_grad_matches_oracle) move the result: the restatement on the oracle's density, run again under five random sign
patterns of that perturbation. A case qualifies if every perturbed run takes the same eta, iteration count and convergence, the
adaptation ELBOs its decisions compare differ by more than 1 % of the larger magnitude, and Y <= 1e-8. Comparisons then hold
10 Y (the five patterns differ among themselves by up to that factor; the response at eta = 1 is not linear)."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import independent as ind
from tests import advi_restate as R

GRAD_TOL = 1e-10                                 # relative to 1 + |g|: test_gpu_parity.test_log_prob_grad_matches_oracle
N_PATTERNS = 5
Y_MAX = 1e-8
ELBO_MARGIN = 0.01


@dataclass(frozen=True)
class Case:
    name: str
    G: int
    S: int
    C: int
    K: int
    data_seed: int
    excluded: bool
    cfg: dict = field(hash=False, compare=False)
    eta: float | None                            # what the case was chosen to reach; None: every step size fails
    iterations: int | None
    converged: bool | None
    reaches: str = ""

    @property
    def D(self):
        return ind.offsets(self.G, self.C, self.K)["D"]

    def data(self):
        """(synth dict, exclusions): the exclusion triple of test_gpu_parity._point"""
        d = ind.synth(self.G, self.S, K=self.K, seed=self.data_seed, C=self.C)
        n = self.G * self.S
        excl = np.array(sorted({1 % n, (2 * self.S + 3) % n, (self.G - 1) * self.S}), dtype=np.int32) if self.excluded else None
        return d, excl

    def full_cfg(self):
        c = dict(output_samples=1000, iter=50000, tol_rel_obj=0.005, elbo_samples=100, eval_elbo=100, adapt_iter=50, seed=1)
        c.update(self.cfg)
        return c


_SHORT = dict(output_samples=8, iter=10, elbo_samples=7, eval_elbo=5, adapt_iter=3, seed=3)
_A_ORIG = dict(output_samples=8, iter=30, elbo_samples=7, eval_elbo=10, adapt_iter=5, seed=3)

CASES = {c.name: c for c in (
    Case("A", 12, 6, 1, 2, 4, False, _SHORT, 0.1, 10, False, "C = 1, nslot = 7"),
    Case("B", 30, 11, 3, 4, 3, True, dict(output_samples=70, iter=10, elbo_samples=40, eval_elbo=5, adapt_iter=3, seed=3),
         1.0, 10, False, "C = 3, ELBO batches 32 + 8, output rows 64 + 6, exclusions"),
    Case("C", 6, 3, 2, 0, 8, False, _A_ORIG, 0.1, 30, False, "K = 0"),
    Case("D", 280, 12, 2, 20, 12, True, dict(output_samples=65, iter=12, elbo_samples=33, eval_elbo=4, adapt_iter=3, seed=5),
         0.1, 12, False, "D = 586: three workgroups, ELBO batches 32 + 1, output rows 64 + 1"),
    Case("E", 40, 10, 2, 4, 21, False, dict(output_samples=8, iter=400, tol_rel_obj=0.05, elbo_samples=20, eval_elbo=20,
                                            adapt_iter=10, seed=3), 1.0, 140, True, "convergence through the buffer"),
    Case("F", 9, 1, 2, 2, 6, False, _A_ORIG, 0.01, 30, False, "S = 1, adapt_eta's last branch"),
    Case("G", 25, 9, 5, 6, 5, False, _SHORT, 0.1, 10, False, "C = 5, continuous columns"),
    Case("H", 40, 10, 2, 4, 21, True, dict(output_samples=8, iter=60, tol_rel_obj=0.3, elbo_samples=20, eval_elbo=10,
                                           adapt_iter=5, seed=7), None, None, None, "every step size fails"),
)}
FITTED = tuple(n for n, c in CASES.items() if c.eta is not None)


def oracle_density(oracle, case):
    d, excl = case.data()
    mo = oracle.model(d["counts"], d["X"], d["exposure"], case.K, excl=excl)
    return lambda z: oracle.log_prob_grad(mo, z)


def sign_pattern(pattern, scale=GRAD_TOL):
    """perturb(g, draw_id) = +-scale (1 + |g|), the signs drawn from a generator seeded by (draw_id, pattern)"""
    def perturb(g, draw_id):
        s = np.random.default_rng([int(draw_id), int(pattern)]).integers(0, 2, size=g.size) * 2.0 - 1.0
        return s * scale * (1.0 + np.abs(g))
    return perturb


def run(case, density, perturb=None):
    """The restatement on a case; None where every step size fails"""
    try:
        return R.advi(density, case.D, R.lp_const(case.G, case.C, case.K), perturb=perturb, **case.full_cfg())
    except R.StepSizeError:
        return None


def distance(a, b):
    """The largest of max |d mu|, max |d omega|, max |d draws| and |d elbo / elbo| between two results"""
    return max(float(np.max(np.abs(a["mu"] - b["mu"]))), float(np.max(np.abs(a["omega"] - b["omega"]))),
               float(np.max(np.abs(a["draws"] - b["draws"]))), abs((a["elbo"] - b["elbo"]) / b["elbo"]))


def elbo_margin(compared):
    """The smallest relative gap among the ELBO pairs adapt_eta compared (two infinite ELBOs decide nothing rounding could move)"""
    m = math.inf
    for a, b in compared:
        if math.isfinite(a) and math.isfinite(b):
            m = min(m, abs(a - b) / max(abs(a), abs(b)))
    return m


def measure(case, density, scale=GRAD_TOL):
    """(the unperturbed result, Y, why the case does not qualify: a list, empty if it does)"""
    base = run(case, density)
    pert = [run(case, density, sign_pattern(p, scale)) for p in range(N_PATTERNS)]
    if base is None:
        return None, 0.0, [] if all(p is None for p in pert) else ["a perturbed run found a step size"]
    why = []
    if any(p is None for p in pert):
        return base, math.inf, ["every step size fails in a perturbed run"]
    for k, p in enumerate(pert):
        if (p["eta"], p["iterations"], p["converged"]) != (base["eta"], base["iterations"], base["converged"]):
            why.append(f"pattern {k}: eta, iterations, converged = {p['eta']}, {p['iterations']}, {p['converged']}")
    margin = min(elbo_margin(r["compared"]) for r in [base] + pert)
    if not margin > ELBO_MARGIN:
        why.append(f"adaptation ELBOs within {margin:.3g} of each other")
    Y = max(distance(p, base) for p in pert) if not why else math.inf
    if not Y <= Y_MAX:
        why.append(f"Y = {Y:.3g}")
    return base, Y, why


@functools.lru_cache(maxsize=None)
def _qualified(name):
    from oracle.oracle import Oracle
    return measure(CASES[name], oracle_density(Oracle(), CASES[name]))


def qualified(name):
    """measure() of a case on the oracle's density, once per process"""
    return _qualified(name)
