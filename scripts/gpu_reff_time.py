"""Cost of the relative efficiency per cell on the MI355X beside the call that uses it: on ONE NUTS fit of a BASELINE cfg3 model
(20 000 genes x 200 samples, 1 000 checked; 8 chains, 150 + 250 iterations: 2 000 kept draws) the checked genes' 200 000 cells
through Fit.loo (r_eff = 1), Fit.relative_eff and Fit.loo(r_eff="auto") -- wall time around the synchronous calls, interleaved,
the median of REPEATS rounds after a warm-up round. A record, not a gate. Writes the JSON line to stdout and to the path given as
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
             relative_eff=lambda: f.relative_eff(checked),
             loo_auto=lambda: f.loo(checked, r_eff="auto"))
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
re = last["relative_eff"]
auto = last["loo_auto"]
thr = 0.7
rec = dict(what="Fit.loo, Fit.relative_eff and Fit.loo(r_eff=\"auto\") of the 1 000 checked genes' cells of one cfg3 NUTS fit "
                "(8 x 250 kept draws): median wall seconds of interleaved synchronous calls",
           n_draws=int(f.chains * f.n_keep), cells=int(K * 200), repeats=REPEATS,
           loo_seconds=round(med["loo"], 5), relative_eff_seconds=round(med["relative_eff"], 5),
           loo_auto_seconds=round(med["loo_auto"], 5),
           relative_eff_over_loo=round(med["relative_eff"] / med["loo"], 4),
           loo_auto_over_sum=round(med["loo_auto"] / (med["loo"] + med["relative_eff"]), 4),
           spread={k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
           r_eff_same_bits_in_auto=bool(np.array_equal(np.where(np.isnan(re), 1.0, re), auto["r_eff"])),
           r_eff_nan=int(np.isnan(re).sum()), r_eff_min=float(np.nanmin(re)), r_eff_median=float(np.nanmedian(re)),
           r_eff_max=float(np.nanmax(re)),
           cells_above_0_7=int((last["loo"]["khat"] > thr).sum()), cells_above_0_7_auto=int((auto["khat"] > thr).sum()))
line = json.dumps(rec)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(line + "\n")
f.close()
m.close()
