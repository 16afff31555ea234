"""Draws evaluated per launch for log_p of the Pareto-k diagnostic (ppcx_fit_advi.hip kPsisSlots), measured on the MI355X: a
BASELINE cfg3 model (D = 41 006), the reference's ADVI call (1 000 output draws), and the first Fit.log_ratios() of a fresh fit
of the same seed per slot count, through the testing build's "psis_slots" hook; the slot counts in two passes of opposite
order. A record, not a gate. Writes the JSON line to stdout and to the path given as the first argument, if any."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ppcseq_amd import _lib as L, build  # noqa: E402
from ppcseq_amd.synth import synth  # noqa: E402

L.use_library(build.build_testing())
d = synth(20000, 200, seed=20253)
m = L.Model(d["counts"], d["X"], d["exposure"], d["K"])
SLOTS = (8, 16, 32, 64, 128)
times = {s: [] for s in SLOTS}
ref = None
worst = 0.0
m.fit_advi(output_samples=50, iter=200, seed=2).close()            # warm-up
for order in (SLOTS, SLOTS[::-1]):
    for s in order:
        L.testing_set("psis_slots", s)
        f = m.fit_advi(output_samples=1000, iter=50000, tol_rel_obj=0.005, seed=1, max_attempts=5)
        t0 = time.perf_counter()
        lp, lg = f.log_ratios()
        times[s].append(time.perf_counter() - t0)
        f.close()
        if ref is None:
            ref = lp
        worst = max(worst, float(np.max(np.abs(lp - ref) / np.maximum(1.0, np.abs(ref)))))
L.testing_set("psis_slots", 0)
rec = dict(what="first Fit.log_ratios() (log_p + log_g, 1 000 draws) of a cfg3 ADVI fit by draws per launch", D=m.D,
           seconds={str(s): [round(t, 4) for t in times[s]] for s in SLOTS}, max_rel_diff_log_p_between_slot_counts=worst)
line = json.dumps(rec)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(line + "\n")
m.close()
