"""The NUTS cases shared by tests/test_nuts_restate.py (CPU) and tests/test_gpu_nuts.py (device), and their qualification: a
case is only compared across implementations if rounding cannot move its decisions ("How NUTS is held").

Trajectories amplify rounding, so no fixed tolerance fits. A case's yardsticks are how far gradient errors of the size the suite
allows the device (1e-10 (1 + |g|), the tolerance of test_log_prob_grad_matches_oracle) move each compared quantity: the
restatement (tests/nuts_restate.py) on the oracle's density, run again under five random sign patterns of that perturbation. A
case qualifies if its integer decisions -- n_leapfrog, treedepth and divergent of every iteration, the iterations of the metric
updates, the number of init attempts -- are the same in those five runs and in five more at 1e-8 (1 + |g|), a margin of 100,
and every yardstick is at most 1e-6. Comparisons then hold 10 times the quantity's yardstick (the patterns differ among
themselves by up to that factor). A case that does not qualify is replaced by another seed, never loosened."""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import independent as ind
from tests import nuts_restate as R

GRAD_TOL = 1e-10                                 # relative to 1 + |g|: test_gpu_parity.test_log_prob_grad_matches_oracle
MARGIN = 100.0                                   # the integer decisions also hold at GRAD_TOL * MARGIN
N_PATTERNS = 5
Y_MAX = 1e-6
HOLD = 10.0
QUANTITIES = ("draws", "lp", "stepsize", "accept", "inv_metric")
INTEGERS = ("n_leapfrog", "treedepth", "divergent")


@dataclass(frozen=True)
class Case:
    name: str
    G: int
    S: int
    C: int
    K: int
    data_seed: int
    excluded: bool
    cfg: dict = field(hash=False, compare=False)   # iter, warmup, seed, max_treedepth and, where not the defaults, the windows
    updates: tuple                               # (iteration, n) of every metric update, derived by hand from the schedule
    chains: int = 2
    chain_id_offset: int = 0
    reaches: str = ""

    @property
    def D(self):
        return ind.offsets(self.G, self.C, self.K)["D"]

    @property
    def hyper(self):
        """The six hyper coordinates: lambda_mu, lambda_sigma, lambda_skew first, the three sigmas last"""
        return (0, 1, 2, self.D - 3, self.D - 2, self.D - 1)

    def data(self):
        """(synth dict, exclusions): the exclusion triple of test_gpu_parity._point"""
        d = ind.synth(self.G, self.S, K=self.K, seed=self.data_seed, C=self.C)
        n = self.G * self.S
        excl = np.array(sorted({1 % n, (2 * self.S + 3) % n, (self.G - 1) * self.S}), dtype=np.int32) if self.excluded else None
        return d, excl


_AUTO = dict(iter=24, warmup=20, seed=11)                                    # 75 + 25 + 50 > 20: 15 % / 10 % -> 3 / 15 / 2
_N2 = dict(iter=28, warmup=24, seed=11, init_buffer=4, window=5, term_buffer=5, max_treedepth=4)
_N3 = dict(iter=24, warmup=20, seed=11, init_buffer=1, window=2, term_buffer=1, max_treedepth=3)
_N4 = dict(iter=24, warmup=20, seed=11, init_buffer=2, window=4, term_buffer=2, max_treedepth=3)
_N6 = dict(iter=24, warmup=20, seed=11, init_buffer=2, window=4, term_buffer=0, max_treedepth=4)

# Update iterations by hand (0-based; a window ends at iteration `next`, and holds the draws of the iterations since the last end
# or since init_buffer): N1 3 + 15 - 1 = 17, the last window's end 20 - 2 - 1. N2 4 + 5 - 1 = 8; doubled, 8 + 10 = 18 = 24 - 5 - 1.
# N3 1 + 2 - 1 = 2; 2 + 4 = 6 (6 + 8 < 19); 6 + 8 = 14, but 14 + 16 >= 19: stretched to 20 - 1 - 1 = 18. N4 2 + 4 - 1 = 5; 5 + 8 = 13,
# 13 + 16 >= 18: stretched to 17. N6 5; 13, 13 + 16 >= 20: stretched to 19, the last warm-up iteration.
CASES = {c.name: c for c in (
    Case("N1", 16, 5, 2, 3, 9, False, dict(_AUTO, seed=1, max_treedepth=3), ((17, 15),), chains=5,
         reaches="automatic schedule 3/15/2, one update, complete_adaptation, kept draws; five chains: two chain groups"),
    Case("N2", 30, 11, 3, 4, 3, True, dict(_N2, seed=3, max_treedepth=3), ((8, 5), (18, 10)),
         reaches="two updates, the second window doubled; C = 3, exclusions; chain 0 starts at its second init attempt"),
    Case("N3", 12, 6, 1, 2, 4, False, dict(_N3, seed=2), ((2, 2), (6, 4), (18, 12)),
         reaches="three updates: doubling, then the stretch to the last window; C = 1"),
    Case("N4", 6, 3, 2, 0, 8, False, _N4, ((5, 4), (17, 12)), reaches="K = 0"),
    Case("N5", 280, 12, 2, 20, 12, True, dict(_AUTO, max_treedepth=3), ((17, 15),),
         reaches="D = 586: coordinates over three workgroups, exclusions"),
    Case("N6", 6, 3, 2, 0, 8, False, _N6, ((5, 4), (19, 14)),
         reaches="term_buffer = 0: update at the last warm-up iteration, then step size exactly 1"),
    Case("N7", 25, 9, 5, 6, 5, False, dict(iter=12, warmup=8, seed=11, max_treedepth=4), (),
         reaches="warmup < 20: dual averaging only, unit metric; C = 5, continuous columns"),
    Case("N8", 9, 1, 2, 2, 6, False, dict(_AUTO, seed=1, max_treedepth=3), ((17, 15),), chains=3, chain_id_offset=3,
         reaches="chain_id_offset = 3, three chains; S = 1"),
)}
ROWS = tuple(CASES)


def oracle_model(oracle, case):
    d, excl = case.data()
    return oracle.model(d["counts"], d["X"], d["exposure"], case.K, excl=excl)


def oracle_density(oracle, case):
    mo = oracle_model(oracle, case)
    return lambda u: oracle.log_prob_grad(mo, u)


def sign_pattern(pattern, D, scale):
    """perturb(g) = +-scale (1 + |g|), one fixed random sign per coordinate"""
    s = np.random.default_rng([int(pattern), 0x4E555453]).integers(0, 2, size=D) * 2.0 - 1.0
    return lambda g: s * scale * (1.0 + np.abs(g))


def run(case, density, perturb=None, faults=()):
    """The restatement on a case: per-chain arrays stacked, the common form of every result compared here"""
    chains = [R.nuts_chain(density, case.D, chain_id=case.chain_id_offset + c, perturb=perturb, faults=faults, hyper=case.hyper,
                           **case.cfg) for c in range(case.chains)]
    out = {k: np.stack([getattr(ch, k) for ch in chains]) for k in QUANTITIES + INTEGERS}
    out["updates"] = [[(it, n) for it, n, _ in ch.metric_updates] for ch in chains]
    out["init_attempts"] = [ch.init_attempts for ch in chains]
    out["metric_history"] = [ch.metric_updates for ch in chains]
    return out


def from_oracle(r):
    out = {k: getattr(r, k) for k in ("draws", "lp", "stepsize", "accept") + INTEGERS}
    out["inv_metric"] = r.metric
    return out


def oracle_run(oracle, case):
    cfg = oracle.cfg(chains=case.chains, **case.cfg)
    return from_oracle(oracle.nuts_model(oracle_model(oracle, case), cfg, chain_id_offset=case.chain_id_offset))


def integer_differences(a, b):
    """The names of the integer decisions in which two results differ"""
    bad = [k for k in INTEGERS if not np.array_equal(a[k], b[k])]
    for k in ("updates", "init_attempts"):
        if k in a and k in b and a[k] != b[k]:
            bad.append(k)
    return bad


def differences(a, b):
    """Per compared quantity, the largest difference of a to b in the quantity's measure"""
    with np.errstate(all="ignore"):
        return dict(draws=float(np.max(np.abs(a["draws"] - b["draws"]))),
                    lp=float(np.max(np.abs(a["lp"] - b["lp"]) / (1.0 + np.abs(b["lp"])))),
                    stepsize=float(np.max(np.abs(a["stepsize"] - b["stepsize"]) / b["stepsize"])),
                    accept=float(np.max(np.abs(a["accept"] - b["accept"]))),
                    inv_metric=float(np.max(np.abs(a["inv_metric"] - b["inv_metric"]) / b["inv_metric"])))


def measure(case, density):
    """(the unperturbed result, the yardsticks, why the case does not qualify: a list, empty if it does)"""
    base = run(case, density)
    why, Y = [], {q: 0.0 for q in QUANTITIES}
    for scale in (GRAD_TOL, GRAD_TOL * MARGIN):
        for p in range(N_PATTERNS):
            r = run(case, density, sign_pattern(p, case.D, scale))
            bad = integer_differences(r, base)
            if bad:
                why.append(f"pattern {p} at {scale:g}: {', '.join(bad)} differ")
            elif scale == GRAD_TOL:
                d = differences(r, base)
                Y = {q: max(Y[q], d[q]) for q in QUANTITIES}
    why += [f"Y[{q}] = {Y[q]:.3g}" for q in QUANTITIES if not Y[q] <= Y_MAX]
    return base, Y, why


def exceeded(a, b, Y):
    """The quantities in which a differs from b by more than HOLD times the yardstick, with the figures"""
    d = differences(a, b)
    return {q: (d[q], HOLD * Y[q]) for q in QUANTITIES if not d[q] <= HOLD * Y[q]}


@functools.lru_cache(maxsize=None)
def _qualified(name):
    from oracle.oracle import Oracle
    return measure(CASES[name], oracle_density(Oracle(), CASES[name]))


def qualified(name):
    """measure() of a case on the oracle's density, once per process"""
    return _qualified(name)
