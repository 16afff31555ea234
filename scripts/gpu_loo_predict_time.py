"""Cost of the leave-one-out predictive intervals on the MI355X beside the two calls whose work they join: on ONE NUTS fit of a
BASELINE cfg3 model (20 000 genes x 200 samples, 1 000 checked; 8 chains, 150 + 250 iterations: 2 000 kept draws) the checked
genes' 200 000 cells through Fit.loo, Fit.ppc and Fit.loo_predict -- wall time around the synchronous calls, interleaved, the
median of REPEATS rounds after a warm-up round. A record, not a gate. Writes the JSON line to stdout and to the path given as
the first argument, if any."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ppcseq_amd import _lib as L  # noqa: E402
from ppcseq_amd.synth import synth  # noqa: E402

REPEATS = 7
d = synth(20000, 200, seed=20253)
K = int(d["K"])
m = L.Model(d["counts"], d["X"], d["exposure"], K)
f = m.fit_nuts(chains=8, iter=400, warmup=150, seed=1)
checked = np.arange(K)
calls = dict(loo=lambda: f.loo(checked),
             ppc=lambda: f.ppc(1.0, 0.025, 0.975, seed=1),
             loo_predict=lambda: f.loo_predict(checked, seed=1))
times = {k: [] for k in calls}
last = {}
for rep in range(REPEATS + 1):                                   # round 0 warms the code objects and the allocator up
    for name, call in calls.items():
        t0 = time.perf_counter()
        last[name] = call()
        dt = time.perf_counter() - t0
        if rep:
            times[name].append(dt)
med = {k: statistics.median(v) for k, v in times.items()}
res = last["loo_predict"]
rec = dict(what="Fit.loo, Fit.ppc and Fit.loo_predict of the 1 000 checked genes' cells of one cfg3 NUTS fit (8 x 250 kept draws): "
                "median wall seconds of interleaved synchronous calls",
           n_draws=int(f.chains * f.n_keep), cells=int(K * 200), repeats=REPEATS,
           loo_seconds=round(med["loo"], 5), ppc_seconds=round(med["ppc"], 5), loo_predict_seconds=round(med["loo_predict"], 5),
           loo_predict_over_sum=round(med["loo_predict"] / (med["loo"] + med["ppc"]), 4),
           spread={k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
           ppc_kernel_ms=round(f.ppc_timing()[0], 3),
           khat_same_bits_as_loo=bool(np.array_equal(res["khat"], last["loo"]["khat"], equal_nan=True)),
           cells_outside=int(res["outside"].sum()), cells_above_0_7=int((res["khat"] > 0.7).sum()))
line = json.dumps(rec)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(line + "\n")
f.close()
m.close()
