"""Cost of PSIS-LOO per observed cell of a NUTS fit on the MI355X: a BASELINE cfg3 model (20 000 genes x 200 samples, 1 000
checked), the driver's NUTS fit (8 chains, 150 + 250 iterations: 2 000 kept draws), then Fit.loo() of the checked genes' 200 000
cells (after a warm-up call on a few genes), twice, and of all 4 million cells. A record, not a gate. Writes the JSON line to
stdout and to the path given as the first argument, if any."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ppcseq_amd import _lib as L  # noqa: E402
from ppcseq_amd.synth import synth  # noqa: E402
from tests import loo_restate as R  # noqa: E402

d = synth(20000, 200, seed=20253)
K = int(d["K"])
m = L.Model(d["counts"], d["X"], d["exposure"], K)
m.fit_nuts(chains=8, iter=60, warmup=40, seed=2).close()          # warm-up: code objects of the fit's kernels loaded
t0 = time.perf_counter()
f = m.fit_nuts(chains=8, iter=400, warmup=150, seed=1)
fit_s = time.perf_counter() - t0
f.loo(np.arange(4))                                              # warm-up of the LOO kernels
checked = np.arange(K)
t0 = time.perf_counter()
a = f.loo(checked)
loo_s = time.perf_counter() - t0
t0 = time.perf_counter()
b = f.loo(checked)
loo2_s = time.perf_counter() - t0
t0 = time.perf_counter()
full = f.loo()
all_s = time.perf_counter() - t0
# cells of a few genes against the restatement, on the device's own log-likelihood
pick = np.unique(np.linspace(0, 19999, 6).astype(int))
ll = f.log_lik(pick).reshape(f.chains * f.n_keep, -1)
ref = R.loo_columns(ll)
worst = 0.0
for i, k in enumerate(R.FIELDS):
    got = full[k][pick].ravel()
    fin = np.isfinite(ref[:, i])
    worst = max(worst, float(np.max(np.abs(got[fin] - ref[fin, i]) / np.maximum(1.0, np.abs(ref[fin, i])))))
kh = full["khat"]
rec = dict(what="Fit.loo() of a cfg3 NUTS fit (8 chains x 250 kept draws): the 1 000 checked genes, then all 20 000",
           n_draws=int(f.chains * f.n_keep), checked_cells=int(K * 200), all_cells=int(20000 * 200),
           fit_seconds=round(fit_s, 3), loo_checked_seconds=round(loo_s, 4), loo_checked_seconds_second_call=round(loo2_s, 4),
           loo_all_seconds=round(all_s, 4), loo_checked_share_of_fit=round(loo_s / fit_s, 4),
           same_bits_second_call=bool(all(np.array_equal(a[k], b[k], equal_nan=True) for k in R.FIELDS)),
           checked_same_bits_in_all_genes_call=bool(all(np.array_equal(a[k], full[k][:K], equal_nan=True) for k in R.FIELDS)),
           cells_checked_vs_restatement=int(ref.shape[0]), max_rel_diff_vs_restatement=worst,
           elpd_loo_checked=a["estimates"]["elpd_loo"], p_loo_checked=a["estimates"]["p_loo"],
           khat_max=float(np.nanmax(kh)), khat_median=float(np.nanmedian(kh)),
           cells_above_0_7=int((kh > 0.7).sum()), checked_cells_above_0_7=int((a["khat"] > 0.7).sum()))
line = json.dumps(rec)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(line + "\n")
f.close()
m.close()
