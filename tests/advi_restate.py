"""numpy restatement of mean-field ADVI as the project runs it (include/ppcx.h ppcx_fit_advi; oracle.advi), written from DESIGN.md
"ADVI" and Stan's published algorithm (Kucukelbir et al. 2017, "Automatic Differentiation Variational Inference", and the
stochastic_gradient_ascent / adapt_eta / calc_ELBO procedures of Stan's advi): float64 only, its own Philox4x32-10 (Salmon et al.,
SC'11), a pluggable log density. It shares no code with ppcseq_amd/csrc or oracle/ppc_oracle.c. Shared by tests/advi_cases.py,
tests/test_advi_restate.py (CPU) and tests/test_gpu_advi.py (device)."""
import math

import numpy as np

TAG_ADVI = 0x41445649                            # 'ADVI', the second key word of every stream here
ETA_SEQUENCE = (100.0, 10.0, 1.0, 0.1, 0.01)
_M32 = np.uint64(0xFFFFFFFF)


class StepSizeError(RuntimeError):
    """adapt_eta: all step sizes failed"""


# ---- random numbers

def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox-4x32 on the counter (c0, c1, c2, c3) under the key (k0, k1); c0 may be an array. Four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def u01(hi, lo):
    """Two words -> a double inside (0, 1): the upper 53 of their 64 bits, centred in their cell"""
    x = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(11)
    return (x.astype(np.float64) + 0.5) / 9007199254740992.0


def seed32(seed):
    """The first key word: the seed's low word, the high word mixed in (a seed below 2^32 is its own key)"""
    seed = int(seed)
    return ((seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF


def eta_draw(D, draw, k0):
    """The D standard normals of Monte-Carlo draw `draw`: coordinates 2j and 2j + 1 are the cosine and the sine of the Box-Muller
    pair of counter (j, draw, 6, 0)."""
    i = np.arange(D)
    r = philox4x32_10(i >> 1, draw, 6, 0, k0, TAG_ADVI)
    rad, t = np.sqrt(-2.0 * np.log(u01(r[0], r[1]))), 2.0 * math.pi * u01(r[2], r[3])
    return np.where(i & 1, rad * np.sin(t), rad * np.cos(t))


def init_point(D, attempt, k0, radius):
    """U(-radius, radius) per coordinate: counter (i, attempt, 0, 0)"""
    r = philox4x32_10(np.arange(D), attempt, 0, 0, k0, TAG_ADVI)
    return (2.0 * u01(r[0], r[1]) - 1.0) * radius


# ---- decisions

class RelBuffer:
    """The circular buffer of relative ELBO changes: converged when their mean or their median is below the tolerance (the median
    of an even count: the mean of the middle two, as the project takes it)."""

    def __init__(self, iter, eval_elbo):
        self.size, self.v = int(max(0.1 * iter / eval_elbo, 2.0)), []

    def push(self, delta):
        self.v.append(delta)
        del self.v[:-self.size]

    def converged(self, tol):
        s, n = sorted(self.v), len(self.v)
        med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
        return sum(self.v) / n < tol or med < tol


def choose_eta(elbo_init, trial, compared=None):
    """adapt_eta's published decision table. trial(eta) is the ELBO after adapt_iter steps of size eta from the initial point (not
    finite: -inf); it is asked in ETA_SEQUENCE's order and only as far as needed. Returns (eta, the trials' ELBOs); `compared`
    collects the pairs whose comparison decided something."""
    compared = [] if compared is None else compared
    best, eta_best, seen = -math.inf, 0.0, []
    for k, eta in enumerate(ETA_SEQUENCE):
        elbo = trial(eta)
        elbo = elbo if math.isfinite(elbo) else -math.inf
        seen.append(elbo)
        compared += [(elbo, best), (best, elbo_init)] if elbo < best else [(elbo, best)]
        if elbo < best and best > elbo_init:         # the last one did better, and better than where we started: take it
            return eta_best, seen
        if k < len(ETA_SEQUENCE) - 1:
            best, eta_best = elbo, eta
        else:
            compared.append((elbo, elbo_init))
            if elbo > elbo_init:
                return eta, seen
            raise StepSizeError("all step sizes failed")


# ---- the algorithm

def lp_const(G, C, K):
    """What oracle/independent.py log_prob_scipy adds back to library densities -- the constants the model's `~` statements drop
    and ADVI's log density keeps -- with the opposite sign: half_log_2pi for each of the six hyper-priors, the G intercepts, the G
    sigma_raw and the (C - 2) K further slopes; log(sd) for the five hyper-priors of scale 2 (scale 1: nothing) and log(2.5) for
    each further slope; log 2 for each of the K Laplace slopes of a design with a second column."""
    n2 = max(C - 2, 0) * K
    back = (6 + G + G + n2) * 0.5 * math.log(2.0 * math.pi) + 5 * math.log(2.0) + n2 * math.log(2.5)
    if C >= 2:
        back += K * math.log(2.0)
    return -back


def advi(log_prob_grad, D, lp_const, *, output_samples, iter, tol_rel_obj, elbo_samples, eval_elbo, adapt_iter, seed,
         init_radius=2.0, perturb=None):
    """log_prob_grad(z) -> (lp, gradient) of the density without lp_const. perturb(g, draw_id) -> what to add to the gradient of
    Monte-Carlo draw draw_id (finite entries only take it). A dict of mu, omega, draws [output_samples, D], iterations, converged,
    elbo, eta, adapt_elbos (the trials adapt_eta ran), elbo_init, compared (the ELBO pairs adapt_eta's decisions rest on) and
    first_output_id (the draw id of draws[0])."""
    k0 = seed32(seed)
    ids = iter_ids()
    st = {}

    def reset():
        st.update(mu=q0.copy(), om=np.zeros(D), hm=np.zeros(D), ho=np.zeros(D))

    def zeta(draw):
        return st["mu"] + np.exp(st["om"]) * eta_draw(D, draw, k0)

    def calc_elbo():
        acc, ok = 0.0, 0
        for _ in range(elbo_samples):
            lp = log_prob_grad(zeta(next(ids)))[0]
            if math.isfinite(lp):
                acc, ok = acc + (lp + lp_const), ok + 1
        if not ok:
            return -math.inf
        return acc / elbo_samples + (0.5 * D * (1.0 + math.log(2.0 * math.pi)) + float(np.sum(st["om"])))

    def grad_at(draw):
        g = np.asarray(log_prob_grad(zeta(draw))[1], dtype=np.float64)
        if perturb is not None:
            fin = np.isfinite(g)
            g = np.where(fin, g + np.where(fin, perturb(np.where(fin, g, 0.0), draw), 0.0), g)
        return draw, g

    def step(eta, it, at):
        draw, g = at
        with np.errstate(all="ignore"):
            gm, go = g, g * eta_draw(D, draw, k0) * np.exp(st["om"]) + 1.0
            ok = np.isfinite(gm) & np.isfinite(go)   # a coordinate without a finite gradient keeps its state
            gm, go = np.where(ok, gm, 0.0), np.where(ok, go, 0.0)
            hm = gm * gm if it == 1 else 0.1 * gm * gm + 0.9 * st["hm"]
            ho = go * go if it == 1 else 0.1 * go * go + 0.9 * st["ho"]
            es = eta / math.sqrt(it)
            st["hm"], st["ho"] = np.where(ok, hm, st["hm"]), np.where(ok, ho, st["ho"])
            st["mu"] = np.where(ok, st["mu"] + es * gm / (1.0 + np.sqrt(hm)), st["mu"])
            st["om"] = np.where(ok, st["om"] + es * go / (1.0 + np.sqrt(ho)), st["om"])
        return grad_at(next(ids))

    for attempt in range(100):
        q0 = init_point(D, attempt, k0, init_radius)
        lp, g = log_prob_grad(q0)
        if math.isfinite(lp) and np.all(np.isfinite(g)):
            break
    else:
        raise RuntimeError("no finite initial point")
    reset()
    elbo_init = calc_elbo()

    def trial(eta):
        at = grad_at(next(ids))
        for it in range(1, adapt_iter + 1):
            at = step(eta, it, at)
        elbo = calc_elbo()
        reset()
        return elbo

    compared = []
    eta, adapt_elbos = choose_eta(elbo_init, trial, compared)
    buf = RelBuffer(iter, eval_elbo)
    elbo, converged, iterations = 0.0, False, 0
    at = grad_at(next(ids))
    for it in range(1, iter + 1):
        at = step(eta, it, at)
        iterations = it
        if it % eval_elbo == 0:
            prev, elbo = elbo, calc_elbo()
            with np.errstate(all="ignore"):
                buf.push(float(np.abs((np.float64(elbo) - prev) / elbo)))
            if buf.converged(tol_rel_obj):
                converged = True
                break
            at = grad_at(next(ids))
    first = next(ids)
    draws = np.stack([zeta(first + r) for r in range(output_samples)])
    return dict(mu=st["mu"], omega=st["om"], draws=draws, iterations=iterations, converged=converged, elbo=elbo, eta=eta,
                adapt_elbos=adapt_elbos, elbo_init=elbo_init, compared=compared, first_output_id=first)


def iter_ids():
    """Draw ids in program order: 1, 2, ..."""
    i = 1
    while True:
        yield i
        i += 1
