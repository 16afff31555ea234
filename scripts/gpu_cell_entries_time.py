"""Wall time of every per-cell entry on one fixed fit, the parent commit's build against this tree's, on the MI355X: a synthetic
model of 1 000 genes (500 checked) x 100 samples with two excluded cells, 4 x 500 draws around the data's own parameters loaded with
Model.fit_from_draws, and an ADVI fit of the same model (2 000 draws) for the three ADVI entries. The two libraries alternate
in one process, PAIRS pairs after a warm-up pair; each entry is one synchronous call. A record, not a gate: an entry counts as
slower where the new median exceeds the parent's by more than twice the larger same-build spread (max - min) of the visit. An
entry that the parent build lacks is recorded with its new times only.

    git worktree add ../parent <commit> && (cd ../parent && python -m ppcseq_amd.build)
    python scripts/gpu_cell_entries_time.py ../parent/ppcseq_amd/libppcx.so [out.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ppcseq_amd import _lib as L  # noqa: E402
from ppcseq_amd.synth import synth  # noqa: E402
from tests import loo_mm_cases  # noqa: E402

PAIRS = 3
G, S, K, CHAINS, KEEP = 1000, 100, 500, 4, 500


def inputs():
    d = synth(G, S, K=K, seed=20262)
    counts = np.array(d["counts"], np.int32)
    dm = loo_mm_cases.dims(G, 2, K)
    rng = np.random.default_rng(5)
    n = CHAINS * KEEP
    u = rng.normal(0.0, 0.05, (n, dm["D"]))
    h = loo_mm_cases.HYPER[None, :] + rng.normal(0.0, 0.02, (n, 6))
    u[:, 0:3], u[:, dm["tail"]:dm["tail"] + 3] = h[:, :3], h[:, 3:]
    u[:, dm["intercept"]:dm["intercept"] + G] = np.log(counts.mean(axis=1) + 1.0)[None, :] + rng.normal(0.0, 0.25, (n, G))
    u[:, dm["alpha1"]:dm["alpha1"] + K] = rng.normal(0.0, 0.3, (n, K))
    u[:, dm["sigma_raw"]:dm["sigma_raw"] + G] = rng.normal(-1.0, 0.3, (n, G))
    return counts, d["X"], d["exposure"], np.ascontiguousarray(u.reshape(CHAINS, KEEP, dm["D"]))


def one_round(path, counts, X, expo, draws):
    """{entry: seconds} of one call each under the library at path (None: this tree's); an entry whose export the library at
    path lacks is left out"""
    lacking = ()
    if path:
        probe = ctypes.CDLL(path)
        lacking = tuple(name for name in L.EXPORTS if not hasattr(probe, name))
    L.use_library(path, lacking=lacking)
    m = L.Model(counts, X, expo, K, lambda_mu_mu=loo_mm_cases.LAMBDA_MU_MU, excl=np.array([3, 7 * S + 1], np.int32))
    f = m.fit_from_draws(draws)
    a = m.fit_advi(output_samples=CHAINS * KEEP, iter=400, eval_elbo=50, seed=4)
    re = np.full((G, S), 0.7)
    calls = dict(relative_eff=lambda: f.relative_eff(), loo=lambda: f.loo(r_eff=re), loo_mcse=lambda: f.loo(r_eff=re, mcse=True),
                 loo_predict=lambda: f.loo_predict(r_eff=re, seed=3), ppc_exact=lambda: f.ppc_exact(),
                 loo_predict_exact=lambda: f.loo_predict_exact(r_eff=re[:K]),
                 loo_moment_match=lambda: f.loo_moment_match(r_eff=re, k_threshold=0.5, max_iters=4),
                 loo_predict_exact_moment_match=lambda: f.loo_predict_exact_moment_match(r_eff=re[:K], k_threshold=0.5, max_iters=4),
                 loo_moment_match_split=lambda: f.loo_moment_match(r_eff=re, k_threshold=0.5, max_iters=4, split=True),
                 loo_predict_exact_moment_match_split=lambda: f.loo_predict_exact_moment_match(r_eff=re[:K], k_threshold=0.5, max_iters=4,
                                                                                               split=True),
                 loo_moment_match_cov=lambda: f.loo_moment_match(r_eff=re, k_threshold=0.5, max_iters=4, cov=True),
                 loo_moment_match_cov_split=lambda: f.loo_moment_match(r_eff=re, k_threshold=0.5, max_iters=4, cov=True, split=True),
                 loo_predict_exact_moment_match_cov=lambda: f.loo_predict_exact_moment_match_cov(r_eff=re[:K], k_threshold=0.5, max_iters=4),
                 loo_predict_exact_moment_match_cov_split=lambda: f.loo_predict_exact_moment_match_cov(r_eff=re[:K], k_threshold=0.5,
                                                                                                       max_iters=4, split=True),
                 loo_approx=lambda: a.loo_approximate_posterior(), loo_predict_approx=lambda: a.loo_predict_approximate_posterior(seed=3),
                 loo_predict_exact_approx=lambda: a.loo_predict_exact_approximate_posterior())
    out = {}
    try:
        for name, call in calls.items():
            if "ppcx_fit_" + name.removesuffix("_split") in lacking:   # the two forms of the one export the parent build may lack
                continue
            t0 = time.perf_counter()
            call()
            out[name] = time.perf_counter() - t0
    finally:
        a.close()
        f.close()
        m.close()
        L.use_library(None)
    return out


def main():
    parent = sys.argv[1]
    data = inputs()
    times = {"parent": {}, "new": {}}
    for rep in range(PAIRS + 1):                                   # pair 0 warms the code objects and the allocator up
        for build, path in (("parent", parent), ("new", None)):
            for name, dt in one_round(path, *data).items():
                if rep:
                    times[build].setdefault(name, []).append(dt)
    rec = dict(what="seconds per synchronous call, parent build against this tree's, alternating in one process; %d genes x %d samples, "
                    "%d checked, %d draws; %d pairs after a warm-up pair" % (G, S, K, CHAINS * KEEP, PAIRS), entries={})
    for name in times["new"]:
        n = times["new"][name]
        if name not in times["parent"]:                                # new with this tree: nothing to compare with
            rec["entries"][name] = dict(new=[round(t, 5) for t in n], new_median=round(statistics.median(n), 5))
            continue
        p = times["parent"][name]
        spread = max(max(p) - min(p), max(n) - min(n))
        rec["entries"][name] = dict(parent=[round(t, 5) for t in p], new=[round(t, 5) for t in n],
                                    parent_median=round(statistics.median(p), 5), new_median=round(statistics.median(n), 5),
                                    margin=round(2 * spread, 5), slower=bool(statistics.median(n) - statistics.median(p) > 2 * spread))
    line = json.dumps(rec)
    print(line)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
