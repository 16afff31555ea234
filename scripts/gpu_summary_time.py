"""Time of Fit.summary() over every column of a BASELINE cfg3 fit (20 000 genes x 200 samples, 8 chains x 250 kept draws) and
lp__, on the MI355X: one warm-up call on a few columns, then the whole summary once (a record, not a gate). Writes the JSON
line to stdout and to the path given as the first argument, if any."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ppcseq_amd import _lib as L  # noqa: E402
from ppcseq_amd.inference import convergence_warnings  # noqa: E402
from ppcseq_amd.synth import synth  # noqa: E402

d = synth(20000, 200, seed=20253)
m = L.Model(d["counts"], d["X"], d["exposure"], d["K"])
chains, per = 8, 250
t0 = time.perf_counter()
f = m.fit_nuts(chains=chains, iter=150 + per, warmup=150, seed=1)
fit_s = time.perf_counter() - t0
f.summary(np.arange(64))                                   # warm-up: code objects loaded, LDS attribute set
t0 = time.perf_counter()
s = f.summary()
sum_s = time.perf_counter() - t0
t0 = time.perf_counter()
s2 = f.summary()
sum2_s = time.perf_counter() - t0
same = all(np.array_equal(s[k], s2[k], equal_nan=True) for k in s)
# columns from every batch of the call, against the numpy restatement of the tests (tests/summary_restate.py)
from tests import summary_restate as R  # noqa: E402
pick = np.unique(np.linspace(0, f.D - 1, 96).astype(int))
xs = f.columns(pick)
bad = 0
for j, c in enumerate(pick):
    ref = R.summary_column(xs[:, :, j])
    for k in R.FIELDS:
        g, r = s[k][c], ref[k]
        ok = (np.isnan(g) and np.isnan(r)) or abs(g - r) <= (1e-9 if k.startswith("ess") else 1e-12) * max(abs(r), 1.0)
        bad += 0 if ok else 1
rec = dict(what="Fit.summary() of every column + lp__ of a cfg3 fit", D=f.D, columns=int(s["column"].size), chains=chains,
           kept_per_chain=per, draws_bytes=8 * chains * per * f.D, fit_seconds=round(fit_s, 3), summary_seconds=round(sum_s, 4), summary_seconds_second_call=round(sum2_s, 4),
           same_bits_second_call=same, columns_checked_vs_restatement=int(pick.size), fields_off_tolerance=bad,
           rhat_max=float(np.nanmax(s["rhat"])), ess_bulk_min=float(np.nanmin(s["ess_bulk"])),
           ess_tail_min=float(np.nanmin(s["ess_tail"])), nan_columns=int(np.isnan(s["rhat"]).sum()),
           warnings=[w.split("\n")[0] for w in convergence_warnings(s, chains)])
line = json.dumps(rec)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(line + "\n")
f.close()
m.close()
