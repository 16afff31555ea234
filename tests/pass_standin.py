"""The recording stand-in for _lib.Model / Fit behind which the tests/test_pass_checks_*_host.py files run a pass on the host:
every call of the model and the fit goes to one `log(name, *args, **kwargs)` callback and returns arrays of the right shape;
what a file records of them, and what the optional reads of a fit return, is that file's `rec` fixture's to say."""
import warnings

import numpy as np

G, S, K = 6, 4, 2
COUNTS = np.random.default_rng(0).integers(5, 50, size=(G, S)).astype(np.int32)
X = np.stack([np.ones(S), np.array([0.0, 1.0, 0.0, 1.0])], axis=1)
PASS = dict(how_many_posterior_draws=300, cores=3, seed=7, launch=(8, 0), adj_prob_theshold=0.05, truncation_compensation=0.7)


def cells(**fields):
    """a read's result: every field [genes, S] filled with its value"""
    return lambda fit, genes, kw: {k: np.full((len(genes), fit.model.S), v) for k, v in fields.items()}


def install(monkeypatch, reads, log=None, poor_sampler=False):
    """replace _lib.Model (and so Fit) by the stand-ins and return what they log to. reads: {method of Fit: result(fit, first
    argument, keywords)}, the optional reads of a fit. log: the callback for every call; without one the log is a list that gets
    (name, genes, keywords) of every read and ("fit_from_draws",) of a pooled fit, nothing else. poor_sampler: diagnostics()
    reports divergences and a saturated tree depth"""
    from ppcseq_amd import _lib
    record = log
    if log is None:
        record = []

        def log(name, *a, **kw):
            if name in reads:
                record.append((name, np.asarray(a[0]).tolist(), kw))
            elif name == "fit_from_draws":
                record.append((name,))

    class Fit:
        def __init__(self, model, chains, n_keep):
            self.model, self.chains, self.n_keep, self.iter = model, chains, n_keep, n_keep + 150

        def ppc(self, *a, **kw):
            log("ppc", *a, **kw)
            ci = np.zeros((self.model.K, self.model.S, 4))
            ci[..., 0], ci[..., 1], ci[..., 3] = 3.0, 1.0, 2.0             # every count lies above the interval
            return (ci, np.zeros((1, self.model.K, self.model.S), np.int32)) if kw.get("return_counts_rng") else ci

        def columns(self, cols):
            log("columns", cols)
            return np.ones((self.chains, self.n_keep, len(cols)))

        def diagnostics(self):
            log("diagnostics")
            shape = (self.chains, self.iter)
            return dict(divergent=np.full(shape, int(poor_sampler), np.int32), treedepth=np.full(shape, 10 if poor_sampler else 3))

        def advi_info(self):
            log("advi_info")
            return dict(iterations=1, converged=True, elbo=0.0, eta=1.0)

        def close(self):
            log("fit.close")

    def read(name, result):
        def method(self, first, **kw):
            log(name, first, **kw)
            return result(self, first, kw)
        return method

    for name, result in reads.items():
        setattr(Fit, name, read(name, result))

    class Model:
        def __init__(self, counts, X, exposure_rate, K, **kw):
            self.G, self.S = np.shape(counts)
            self.K = int(K)
            log("Model", (self.G, self.S), self.K, **kw)

        def set_exclusions(self, excl):
            log("set_exclusions", np.asarray(excl))

        def set_launch(self, *a):
            log("set_launch", *a)

        def fit_nuts(self, **kw):
            log("fit_nuts", **kw)
            return Fit(self, kw["chains"], kw["iter"] - kw["warmup"])

        def fit_advi(self, **kw):
            log("fit_advi", **kw)
            return Fit(self, 1, kw["output_samples"])

        def fit_from_draws(self, draws):
            log("fit_from_draws", np.shape(draws))
            return Fit(self, draws.shape[0], draws.shape[1])

        def close(self):
            log("model.close")

    monkeypatch.setattr(_lib, "Model", Model)
    monkeypatch.setattr(_lib, "device_memory", lambda device=0: (1 << 40, 1 << 40))
    return record


def run_pass(n_checked=K, **kw):
    """(do_inference's result over COUNTS with PASS and kw, the warnings it raised)"""
    from ppcseq_amd.inference import do_inference
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = do_inference(COUNTS, X, np.zeros(S), n_checked, **{**PASS, **kw})
    return res, w
