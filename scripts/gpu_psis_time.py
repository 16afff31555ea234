"""Cost of the Pareto-k diagnostic of an ADVI fit on the MI355X: a BASELINE cfg3 model (20 000 genes x 200 samples, D = 41 006),
the reference's ADVI call (1 000 output draws, tol_rel_obj 0.005), then log_p + log_g at the kept draws (the first
Fit.log_ratios(), synchronous) and Fit.psis() over every column and the log ratios (after a warm-up call on a few columns), twice.
A record, not a gate. Writes the JSON line to stdout and to the path given as the first argument, if any."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ppcseq_amd import _lib as L  # noqa: E402
from ppcseq_amd.synth import synth  # noqa: E402
from tests import psis_restate as R  # noqa: E402

d = synth(20000, 200, seed=20253)
m = L.Model(d["counts"], d["X"], d["exposure"], d["K"])
m.fit_advi(output_samples=50, iter=200, seed=2).close()          # warm-up: code objects of the fit's kernels loaded
t0 = time.perf_counter()
f = m.fit_advi(output_samples=1000, iter=50000, tol_rel_obj=0.005, seed=1, max_attempts=5)
fit_s = time.perf_counter() - t0
t0 = time.perf_counter()
lp, lg = f.log_ratios()
ratios_s = time.perf_counter() - t0
f.psis(np.arange(64))                                             # warm-up of the PSIS kernel
t0 = time.perf_counter()
k = f.psis()
psis_s = time.perf_counter() - t0
t0 = time.perf_counter()
k2 = f.psis()
psis2_s = time.perf_counter() - t0
# columns from every part of the call and the overall k-hat, against the restatement of the tests
r = R.log_ratios(lp, lg)
pick = np.unique(np.linspace(0, f.D - 1, 96).astype(int))
xs = f.columns(pick).reshape(-1, pick.size)
worst = 0.0
for j, c in enumerate(pick):
    ref, got = R.khat(R.column_values(xs[:, j], r)), k["khat"][c]
    worst = max(worst, 0.0 if (got == ref or (np.isnan(ref) and np.isnan(got))) else abs(got - ref) / abs(ref))
ref = R.khat(r)
worst = max(worst, abs(k["khat"][-1] - ref) / abs(ref))
kh = k["khat"][:-1]
rec = dict(what="log_p + log_g and Fit.psis() of every column + the log ratios of a cfg3 ADVI fit (1 000 draws)", D=f.D,
           columns=int(k["column"].size), fit_seconds=round(fit_s, 3), log_ratios_seconds=round(ratios_s, 4),
           psis_seconds=round(psis_s, 4), psis_seconds_second_call=round(psis2_s, 4),
           diagnostic_share_of_fit=round((ratios_s + psis_s) / fit_s, 4),
           same_bits_second_call=bool(np.array_equal(k["khat"], k2["khat"], equal_nan=True)),
           columns_checked_vs_restatement=int(pick.size) + 1, max_rel_diff_vs_restatement=worst,
           khat_overall=float(k["khat"][-1]), khat_columns_max=float(np.nanmax(kh)), khat_columns_median=float(np.nanmedian(kh)),
           columns_above_0_7=int((kh > 0.7).sum()), log_p_finite=int(np.isfinite(lp).sum()), iterations=f.advi_info()["iterations"])
line = json.dumps(rec)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(line + "\n")
f.close()
m.close()
