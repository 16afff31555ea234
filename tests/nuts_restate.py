"""numpy restatement of the NUTS sampler and its warm-up as the project runs them, written from that section
and Stan's published procedure (Hoffman & Gelman 2014; Betancourt 2017, "A Conceptual Introduction to Hamiltonian Monte Carlo";
the base_nuts::transition / build_tree, base_hmc::init_stepsize, stepsize_adaptation, windowed_adaptation, var_adaptation and
welford_var_estimator procedures of Stan's mcmc library): recursive, float64 only, a pluggable density, the Philox4x32-10 and
Box-Muller of tests/advi_restate.py addressed by section 4's "RNG specification". It shares no code with ppcseq_amd/csrc (whose
tree is iterative, on slots) or oracle/ppc_oracle.c. Shared by tests/nuts_cases.py, tests/test_nuts_restate.py (CPU) and
tests/test_gpu_nuts.py (device)."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests.advi_restate import philox4x32_10, seed32, u01

MAX_DELTA_H = 1000.0
LOG_08 = math.log(0.8)

# Faults a test may seed (tests/test_nuts_restate.py only): each is one of the silent mistakes the comparisons exist to catch.
FAULTS = ("welford_n", "regulariser", "set_mu", "no_restart", "eps_call", "no_doubling", "hyper_unit", "no_complete")


class InitError(RuntimeError):
    """no finite initial point in 100 attempts"""


# ---- random numbers ("RNG specification")

class Streams:
    def __init__(self, seed, chain_id, D):
        self.k0, self.k1, self.i = seed32(seed), int(chain_id) & 0xFFFFFFFF, np.arange(D)

    def _first(self, c0, c1, c2, c3=0):
        r = philox4x32_10(c0, c1, c2, c3, self.k0, self.k1)
        return u01(r[0], r[1])

    def init_uniforms(self, attempt):
        return self._first(self.i, attempt, 0)

    def _normals(self, c1, c2, c3):
        """Coordinates 2j and 2j + 1 are the cosine and the sine of the Box-Muller pair of counter (j, c1, c2, c3)"""
        r = philox4x32_10(self.i >> 1, c1, c2, c3, self.k0, self.k1)
        rad, t = np.sqrt(-2.0 * np.log(u01(r[0], r[1]))), 2.0 * math.pi * u01(r[2], r[3])
        return np.where(self.i & 1, rad * np.sin(t), rad * np.cos(t))

    def momenta(self, it):
        return self._normals(it, 1, 0)

    def search_momenta(self, call, attempt):
        return self._normals(call, 3, attempt)

    def scalar(self, j, it):
        return float(self._first(j, it, 2))

    def goes_forward(self, depth, it):
        return float(self._first(depth, it, 7)) > 0.5


# ---- the Hamiltonian system: diagonal Euclidean metric, leapfrog

@dataclass
class Point:
    q: np.ndarray
    p: np.ndarray
    V: float                                     # potential: minus the log density
    dV: np.ndarray

    def copy(self):
        return Point(self.q.copy(), self.p.copy(), self.V, self.dV.copy())


class System:
    def __init__(self, density, D, perturb=None):
        self.density, self.perturb, self.minv = density, perturb, np.ones(D)

    def potential(self, q):
        lp, g = self.density(q)
        g = np.asarray(g, dtype=np.float64)
        if self.perturb is not None:
            fin = np.isfinite(g)
            g = np.where(fin, g + self.perturb(np.where(fin, g, 0.0)), g)
        return -float(lp), -g

    def at(self, q, p=None):
        V, dV = self.potential(q)
        return Point(q.copy(), np.zeros_like(q) if p is None else p, V, dV)

    def H(self, z):
        h = z.V + 0.5 * float(np.dot(z.p, self.minv * z.p))
        return math.inf if math.isnan(h) else h

    def leapfrog(self, z, eps):
        p = z.p - 0.5 * eps * z.dV
        q = z.q + eps * (self.minv * p)
        V, dV = self.potential(q)
        return Point(q, p - 0.5 * eps * dV, V, dV)


def log_sum_exp(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def no_u_turn(sharp_minus, sharp_plus, rho):
    return float(np.dot(sharp_plus, rho)) > 0 and float(np.dot(sharp_minus, rho)) > 0


# ---- one transition

@dataclass
class Tree:
    """What build_tree hands up: the subtree's ends in time order of its construction, its summed momenta and log weight, the
    state it proposes and the state it stopped at."""
    valid: bool
    z_end: Point = None
    propose: Point = None
    p_beg: np.ndarray = None
    p_end: np.ndarray = None
    sharp_beg: np.ndarray = None
    sharp_end: np.ndarray = None
    rho: np.ndarray = None
    lsw: float = -math.inf


class Transition:
    def __init__(self, sysm, streams, it, eps, z0):
        self.s, self.rng, self.it, self.eps = sysm, streams, it, eps
        self.H0 = sysm.H(z0)
        self.n_leapfrog, self.sum_metro, self.divergent, self.j = 0, 0.0, False, 0

    def uniform(self):
        self.j += 1
        return self.rng.scalar(self.j - 1, self.it)

    def build(self, depth, z, sign):
        if depth == 0:
            z1 = self.s.leapfrog(z, sign * self.eps)
            self.n_leapfrog += 1
            dH = self.H0 - self.s.H(z1)
            if -dH > MAX_DELTA_H:
                self.divergent = True
            self.sum_metro += 1.0 if dH > 0 else math.exp(dH)
            sharp = self.s.minv * z1.p
            return Tree(not self.divergent, z1, z1, z1.p, z1.p, sharp, sharp, z1.p.copy(), dH)
        a = self.build(depth - 1, z, sign)
        if not a.valid:
            return Tree(False)
        b = self.build(depth - 1, a.z_end, sign)
        if not b.valid:
            return Tree(False)
        lsw = log_sum_exp(a.lsw, b.lsw)
        propose = a.propose
        if b.lsw > lsw or self.uniform() < math.exp(b.lsw - lsw):
            propose = b.propose
        rho = a.rho + b.rho
        ok = (no_u_turn(a.sharp_beg, b.sharp_end, rho)
              and no_u_turn(a.sharp_beg, b.sharp_beg, a.rho + b.p_beg)
              and no_u_turn(a.sharp_end, b.sharp_end, b.rho + a.p_end))
        return Tree(ok, b.z_end, propose, a.p_beg, b.p_end, a.sharp_beg, b.sharp_end, rho, lsw)

    def run(self, z0, max_depth):
        """-> (the sample, depth). The trajectory's two ends; `old` is everything built so far as one subtree from its backward
        to its forward end."""
        sharp0 = self.s.minv * z0.p
        bck = fwd = z0
        old = Tree(True, None, z0, z0.p, z0.p, sharp0, sharp0, z0.p.copy(), 0.0)
        sample, depth = z0, 0
        while depth < max_depth:
            forward = self.rng.goes_forward(depth, self.it)
            new = self.build(depth, fwd if forward else bck, 1 if forward else -1)
            if not new.valid:
                break
            if forward:
                fwd = new.z_end
                lo, hi = old, new                # backward part, forward part, each with beg = its backward end
            else:
                bck = new.z_end                  # built backwards in time: its beginning is its forward end
                lo = Tree(True, None, None, new.p_end, new.p_beg, new.sharp_end, new.sharp_beg, new.rho, new.lsw)
                hi = old
            depth += 1
            if new.lsw > old.lsw or self.uniform() < math.exp(new.lsw - old.lsw):
                sample = new.propose
            rho = lo.rho + hi.rho
            persist = (no_u_turn(lo.sharp_beg, hi.sharp_end, rho)
                       and no_u_turn(lo.sharp_beg, hi.sharp_beg, lo.rho + hi.p_beg)
                       and no_u_turn(lo.sharp_end, hi.sharp_end, hi.rho + lo.p_end))
            old = Tree(True, None, None, lo.p_beg, hi.p_end, lo.sharp_beg, hi.sharp_end, rho, log_sum_exp(old.lsw, new.lsw))
            if not persist:
                break
        return sample, depth


# ---- adaptation

class DualAveraging:
    gamma, t0, kappa = 0.05, 10.0, 0.75

    def __init__(self, delta):
        self.delta, self.mu = delta, 0.0
        self.restart()

    def restart(self):
        self.counter, self.s_bar, self.x_bar = 0, 0.0, 0.0

    def learn(self, accept):
        self.counter += 1
        eta = 1.0 / (self.counter + self.t0)
        self.s_bar = (1.0 - eta) * self.s_bar + eta * (self.delta - min(accept, 1.0))
        x = self.mu - self.s_bar * math.sqrt(self.counter) / self.gamma
        x_eta = self.counter ** -self.kappa
        self.x_bar = (1.0 - x_eta) * self.x_bar + x_eta * x
        return math.exp(x)

    def complete(self):
        return math.exp(self.x_bar)


class Windows:
    """windowed_adaptation: which warm-up iterations feed the variance estimate, and at which of them a window ends"""

    def __init__(self, warmup, init_buffer, term_buffer, window, faults=()):
        self.on = warmup >= 20
        if self.on and init_buffer + window + term_buffer > warmup:
            init_buffer, term_buffer = int(0.15 * warmup), int(0.1 * warmup)
            window = warmup - (init_buffer + term_buffer)
        self.warmup, self.init_buffer, self.term_buffer, self.faults = warmup, init_buffer, term_buffer, faults
        self.counter, self.size, self.next = 0, window, init_buffer + window - 1

    @property
    def last(self):
        return self.warmup - self.term_buffer - 1

    def inside(self):
        return self.on and self.init_buffer <= self.counter < self.warmup - self.term_buffer

    def ends(self):
        return self.on and self.counter == self.next and self.counter != self.warmup

    def compute_next(self):
        if self.next == self.last:
            return
        if "no_doubling" not in self.faults:
            self.size *= 2
        self.next = self.counter + self.size
        if self.next == self.last:
            return
        if self.next + 2 * self.size >= self.warmup - self.term_buffer:
            self.next = self.last


class Welford:
    def __init__(self, D):
        self.D = D
        self.restart()

    def restart(self):
        self.n, self.m, self.m2 = 0, np.zeros(self.D), np.zeros(self.D)

    def add(self, q):
        self.n += 1
        delta = q - self.m
        self.m = self.m + delta / self.n
        self.m2 = self.m2 + (q - self.m) * delta

    def variance(self):
        return self.m2 / (self.n - 1.0)


def init_stepsize(sysm, streams, z, eps, call):
    """The step size at which one leapfrog from z with fresh momenta crosses an acceptance of 0.8, by doubling or halving"""
    if eps == 0 or eps > 1e7 or math.isnan(eps):
        return eps
    attempt, direction = 0, 0
    while True:
        z0 = Point(z.q, streams.search_momenta(call, attempt) / np.sqrt(sysm.minv), z.V, z.dV)
        attempt += 1
        dH = sysm.H(z0) - sysm.H(sysm.leapfrog(z0, eps))
        if direction == 0:
            direction = 1 if dH > LOG_08 else -1
            continue
        if direction == 1 and not dH > LOG_08:
            return eps
        if direction == -1 and not dH < LOG_08:
            return eps
        eps = 2.0 * eps if direction == 1 else 0.5 * eps
        if eps > 1e7 or eps == 0:
            return eps


@dataclass
class Chain:
    draws: np.ndarray
    lp: np.ndarray
    stepsize: np.ndarray
    treedepth: np.ndarray
    n_leapfrog: np.ndarray
    divergent: np.ndarray
    accept: np.ndarray
    init_attempts: int
    metric_updates: list = field(default_factory=list)   # (iteration, n, the inverse metric after the update)

    @property
    def update_iterations(self):
        return [it for it, _, _ in self.metric_updates]

    @property
    def inv_metric(self):
        return self.metric_updates[-1][2] if self.metric_updates else np.ones(self.draws.shape[1])


def nuts_chain(density, D, *, iter, warmup, seed, chain_id=0, adapt_delta=0.8, max_treedepth=10, init_radius=2.0, stepsize0=1.0,
               init_buffer=75, term_buffer=50, window=25, perturb=None, faults=(), hyper=()):
    """density(u) -> (lp, gradient). perturb(g) -> what to add to a gradient (finite entries only take it). faults: names out of
    FAULTS; hyper: the coordinates the fault "hyper_unit" leaves at 1 in the metric."""
    assert set(faults) <= set(FAULTS), faults
    rng, sysm = Streams(seed, chain_id, D), System(density, D, perturb)
    for attempt in range(100):
        z = sysm.at((2.0 * rng.init_uniforms(attempt) - 1.0) * init_radius)
        if math.isfinite(z.V) and np.all(np.isfinite(z.dV)):
            break
    else:
        raise InitError("no finite initial point")
    nk = iter - warmup
    out = Chain(np.zeros((nk, D)), np.zeros(nk), np.zeros(iter), np.zeros(iter, np.int32), np.zeros(iter, np.int32),
                np.zeros(iter, np.int32), np.zeros(iter), attempt + 1)
    da, win, est = DualAveraging(adapt_delta), Windows(warmup, init_buffer, term_buffer, window, faults), Welford(D)
    search_calls = 0

    def search(eps):
        nonlocal search_calls
        eps = init_stepsize(sysm, rng, z, eps, search_calls)
        if "eps_call" not in faults:
            search_calls += 1
        da.mu = math.log(eps if "set_mu" in faults else 10.0 * eps)
        return eps

    eps = search(stepsize0)
    for it in range(iter):
        z = Point(z.q, rng.momenta(it) / np.sqrt(sysm.minv), z.V, z.dV)
        tr = Transition(sysm, rng, it, eps, z)
        z, depth = tr.run(z, max_treedepth)
        accept = tr.sum_metro / tr.n_leapfrog
        out.stepsize[it], out.treedepth[it], out.n_leapfrog[it] = eps, depth, tr.n_leapfrog
        out.divergent[it], out.accept[it] = tr.divergent, accept
        if it < warmup:
            eps = da.learn(accept)
            if win.inside():
                est.add(z.q)
            if win.ends():
                win.compute_next()
                n = est.n + 1 if "welford_n" in faults else est.n
                var = est.m2 / (n - 1.0)
                minv = (n / (n + 5.0)) * var + (1e-2 if "regulariser" in faults else 1e-3) * (5.0 / (n + 5.0))
                if "hyper_unit" in faults:
                    minv[list(hyper)] = 1.0
                sysm.minv = minv
                out.metric_updates.append((it, est.n, minv.copy()))
                est.restart()
                eps = search(eps)
                if "no_restart" not in faults:
                    da.restart()
            win.counter += 1
            if it == warmup - 1 and "no_complete" not in faults:
                eps = da.complete()
        else:
            out.draws[it - warmup], out.lp[it - warmup] = z.q, -z.V
    return out
