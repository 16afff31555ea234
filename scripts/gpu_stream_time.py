"""Kernel-level timing of the log-likelihood launch on its two routes (development aid): the per-sample constants in LDS against
streamed from global memory (Model(per_sample=...)), timed in interleaved rounds as scripts/gpu_kbench.py does; minimum, median
and maximum per configuration. G, S: the shape (default 20 000 x 200, BASELINE cfg3); ROUTES: lds,stream; CFGS: chains:lanes,..."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppcseq_amd import _lib as L
from ppcseq_amd import build as _b
L.use_library(os.environ.get("PPCX_LIB") or _b.build_testing())          # kernel-level timing lives in the testing build
from ppcseq_amd.synth import synth
G, S = int(os.environ.get("G", 20000)), int(os.environ.get("S", 200))
routes = os.environ.get("ROUTES", "lds,stream").split(",")
cfgs = [tuple(int(v) for v in c.split(":")) for c in os.environ.get("CFGS", "8:8,3:4").split(",")]
d = synth(G, S, seed=20253)
models = {r: L.Model(d["counts"], d["X"], d["exposure"], d["K"], per_sample=r) for r in routes}
reps = int(os.environ.get("REPS", 100))
res = {(r, c): [] for r in routes for c in cfgs}
for rnd in range(int(os.environ.get("ROUNDS", 5))):
    for cfg in cfgs:
        for r in routes:
            models[r].set_launch(cfg[1], 0)
            ms, _ = models[r].bench_kernel(0, cfg[0], 10 if rnd else 40, reps, 1)
            res[r, cfg].append(ms)
out = []
for (r, cfg), ms in res.items():
    ms = 1e3 * np.array(ms)
    out.append(dict(G=G, S=S, route=models[r].per_sample, chains=cfg[0], lanes=cfg[1], launch=models[r].get_launch(),
                    us_min=round(float(ms.min()), 2), us_median=round(float(np.median(ms)), 2), us_max=round(float(ms.max()), 2)))
    print(json.dumps(out[-1]), flush=True)
for m in models.values():
    m.close()
