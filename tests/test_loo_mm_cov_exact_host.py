"""The exact leave-one-out predictive under the weights of the matching with the covariance step without a GPU: the CPU build of
the kernel's header (ppcseq_amd/csrc/ppcx_loo_mm_cov_exact.h: loo_mm_cov_exact_cell_host; tests/loo_mm_cov_exact_cpu) against the
numpy / scipy restatement (tests/loo_mm_cov_exact_restate.py) on the checked-gene cells of tests/loo_mm_cov_exact_cases.py, split
both ways; the record against the CPU builds of the sibling headers (the covariance matching's record bit for bit, the plain
exact predictive where nothing was matched, the diagonal predictive where no covariance step was taken, the held-out density
p_le + p_ge - 1 against the matching's elpd_loo); an invalid transformed draw; the n <= d prefixes; and the factor4 cell against a
held-out reference. The modifier of inference.MODIFIERS is held in tests/test_pass_checks_loo_mm_cov_exact_host.py.

Tolerances. Integer fields equal on cells that qualify (loo_mm_cov_restate.qualifies); lower / upper may be one count apart only
where the restatement's own F at the count between them is within the bound of p, and at most one end over all cells may use
that (none does: the nearest |F - p| over the 58 cell / split pairs is 2.4e-9); values that are not finite in the same places;
the reals at ten times the largest error measured on the cells (X.MEASURED, printed by test_cpu_build_matches_restatement), never
above 1e-9. The restatement inverts the final transform where the header accumulates the inverse step by step.

The factor4 cell (set factor4, gene 0, sample 5, count 2500, d = 5; tc = 1, p = 0.025 / 0.975, 1 000 draws; test_factor4_cell
prints the figures):
                                        khat   mean   lower  upper  log P(X >= y)
  plain PSIS                            1.30   664.8  141    1802   -4.67
  matching of ppcx_loo_mm.h             1.01   343.5  74     957    -6.48
  with the covariance candidate         0.70   163.9  39     449    -10.64
  with it and split (khat_split 0.80)          163.9  40     451    -8.90
  held-out reference                           129.6 +- 0.23  26  385.3 +- 1.2  -9.35 +- 0.16
(60 000 chains of wide_design_cases.metropolis with the cell excluded, in ten batches)."""
import numpy as np
import pytest

from tests import loo_exact_restate as XR
from tests import loo_mm_cases as cases
from tests import loo_mm_cov_exact_cases as K
from tests import loo_mm_cov_exact_restate as X
from tests import loo_mm_cov_restate as V
from tests import loo_mm_exact_restate as E
from tests import loo_mm_restate as R
from tests import loo_mm_split_restate as SP
from tests import wide_design_cases as wide

BOUND = min(10 * X.MEASURED, X.BOUND)
NH = len(X.HEAD)


@pytest.fixture(scope="module")
def host():
    return X.host_lib()


@pytest.fixture(scope="module")
def cov_host():
    return V.host_lib()


@pytest.fixture(scope="module")
def records(host):
    """the CPU build's record of every cell, split both ways: {(cell index, split): record}; computed once and left unchanged"""
    return {(j, split): X.host_cell(host, K.gene_of(c), c["s"], split=split, **K.kw(c)) for j, c in enumerate(K.CELLS)
            for split in (False, True)}


def test_cells_cover_the_paths():
    kinds = [c["kinds"] for c in K.CELLS]
    widths = {K.gene_of(c)["T"].shape[0] for c in K.CELLS if 3 in c["kinds"]}
    assert len(K.CELLS) == 29 and len(K.UNCHECKED) == 5
    per_width = {}
    for c in K.CELLS:
        if 3 in c["kinds"]:
            nc = K.gene_of(c)["T"].shape[0]
            per_width[nc] = per_width.get(nc, 0) + 1
    # 22 paths with a covariance step: 19 at C + 1 = 4, 5, 9, 16, 17 and three at C + 1 = 3 (the sets "b" and "c, planted")
    assert per_width == {3: 3, 4: 1, 5: 4, 9: 5, 16: 2, 17: 7} and sum(per_width.values()) == 22 and widths >= {5, 4, 9, 16, 17}
    assert [2, 3, 2, 2, 1, 2, 1, 2, 3, 3] in kinds                    # later 2s and 3s
    assert sum(c["max_iters"] == 2 and c["kinds"] == [1, 3] for c in K.CELLS) == 2   # stopped by max_iters, at d = 5 and d = 17
    assert sum(k == [] for k in kinds) == 4                           # unmatched: refused at once, two excluded cells, max_iters = 0


def test_cpu_build_matches_restatement(records):
    worst, allowed, per_width = 0.0, [], {}
    for j, c in enumerate(K.CELLS):
        gene = K.gene_of(c)
        nc = gene["T"].shape[0]
        mm = V.point(gene, c["s"], **K.kw(c))
        assert mm["kinds"] == c["kinds"], (c["name"], mm["kinds"])
        assert V.qualifies(gene, c["s"], mm, **K.kw(c)), c["name"]
        for split in (False, True):
            ref = X.point(gene, c["s"], split=split, **K.kw(c))
            got = records[j, split]
            assert got.size == X.fields(nc - 1)
            assert np.isfinite(ref["mean"]) and np.all(np.isfinite(got[:6])), (c["name"], split)   # valid draws, finite statistics
            if X.check_integers(got, ref, BOUND, (c["name"], split)):
                allowed.append((c["name"], split))
            assert np.isnan(got[13]) == (not split or got[11] == 0), (c["name"], split)
            err = X.errors(got, ref)
            print(c["name"], "split", split, "kinds", c["kinds"], "khat", got[10], "->", got[9], "khat_split", got[13], "mean", got[0],
                  "interval", got[4], got[5], "error", err)
            worst = max(worst, err)
            per_width[nc] = max(per_width.get(nc, 0.0), err)
            assert err <= BOUND, (c["name"], split, err)
    print("largest error against the restatement:", worst, "per width C + 1:", per_width, "; interval ends within the bound of p:", allowed)
    assert len(allowed) <= 1, allowed
    assert worst <= X.MEASURED                                        # the recorded value is the measured one


def test_record_against_the_sibling_builds(records, cov_host):
    """khat, khat_before, iterations, cov_iterations, transform and shift are loo_mm_cov_cell_host's bits; a cell with
    iterations == 0 holds loo_exact_cell_host's ten fields bit for bit; a cell with cov_iterations == 0 holds the diagonal
    predictive's record within the bound; p_le + p_ge - 1 is exp(elpd_loo) of the covariance matching"""
    exact_host, diag_host, split_host = XR.host_lib(), E.host_lib(), SP.host_lib()
    unmatched = diagonal = 0
    for j, c in enumerate(K.CELLS):
        gene = K.gene_of(c)
        nc = gene["T"].shape[0]
        for split in (False, True):
            got = records[j, split]
            rec, kinds, _ = V.host_cell(cov_host, gene, c["s"], split=split, **K.kw(c))
            what = (c["name"], split)
            assert np.array_equal(got[[9, 10, 11, 12]], rec[[3, 4, 5, 6]], equal_nan=True), what
            assert np.array_equal(got[NH:], rec[len(V.HEAD):]), what
            if split:
                assert np.array_equal(got[13], rec[8], equal_nan=True), what     # the accumulated inverse on both sides
            density = got[2] + got[3] - 1.0
            d = abs(density - np.exp(rec[0]))
            print(c["name"], "split", split, "p_le + p_ge - 1", density, "exp(elpd_loo)", np.exp(rec[0]), "difference", d)
            assert d <= 2 * BOUND, what
            if got[11] == 0:
                eta, sg, ll = E.host_columns(diag_host, gene, c["s"])
                plain, _ = XR.host_cell(exact_host, ll, eta, sg, int(gene["y"][c["s"]]), excluded=bool(gene["excl"][c["s"]]),
                                        r_eff=c["r_eff"], tc=1.0, p_lo=0.025, p_hi=0.975)
                assert np.array_equal(got[:10], plain, equal_nan=True), what
                unmatched += 1
            if got[12] == 0:
                dg = (SP.host_exact_cell(split_host, gene, c["s"], **K.kw(c)) if split else E.host_cell(diag_host, gene, c["s"], **K.kw(c)))
                tr = got[NH:NH + nc * nc].reshape(nc, nc)
                assert np.all(tr[~np.eye(nc, dtype=bool)] == 0.0), what
                mine = np.concatenate([got[:12], np.diag(tr), got[NH + nc * nc:], got[13:14] if split else []])
                assert all(mine[i] == dg[i] or (np.isnan(mine[i]) and np.isnan(dg[i])) for i in (4, 5, 6, 7, 8, 11)), (what, mine[:12], dg[:12])
                assert np.array_equal(np.isnan(mine), np.isnan(dg)) and np.array_equal(np.isinf(mine), np.isinf(dg)), what
                err = max(X._err(a, b, i in (2, 3)) for i, (a, b) in enumerate(zip(mine, dg)))
                assert err <= BOUND, (what, err)
                diagonal += 1
    print("unmatched", unmatched, "without a covariance step", diagonal)
    assert unmatched >= 6 and diagonal >= 12


def test_invalid_transformed_draw_is_a_nan_record(host):
    """the factor4 cell at a truncation compensation under which every original draw has a finite phi = tc exp(-sigma_raw)
    (the largest is exp(709.7)) while the matching, which moves sigma_raw down by 0.6, takes a transformed draw's past the
    largest double: the matching itself does not read tc, so the cell is matched as ever, and every statistic of the cell is NaN,
    khat and khat_split included; y, excluded and the matching's state stay. (At such a phi the plain predictive is NaN as well,
    by its continued fraction's cap: what is held here is where the matched path ends, with khat.)"""
    gene = cases.gene_of(wide.draw_set("factor4"), 0)
    s = 5
    sg = np.asarray(gene["T"], float)[-1]
    tc = float(np.exp(709.7 + sg.min()))
    for split in (False, True):
        ref = X.point(gene, s, split=split, tc=tc)
        moved = V.transformed(gene, ref["transform"], ref["shift"])[-1]
        assert np.all(np.isfinite(tc * np.exp(-sg))) and moved[:sg.size // 2].min() < sg.min() - 0.1
        got = X.host_cell(host, gene, s, split=split, tc=tc)
        print("split", split, "kinds", ref["kinds"], "iterations", got[11], "record", got[:NH])
        assert ref["kinds"] == [1, 3, 1] and got[11] == 3 and got[12] == 1
        assert np.isnan(ref["mean"]) and np.isnan(ref["khat"]) and np.isnan(ref["khat_split"])
        assert np.all(np.isnan(got[[0, 1, 2, 3, 4, 5, 8, 9, 13]])) and got[6] == gene["y"][s] and got[7] == 0, got[:NH]
        assert np.all(np.isfinite(got[NH:])) and np.isfinite(got[10])
        assert np.array_equal(got[10:13], X.host_cell(host, gene, s, split=split)[10:13])


@pytest.mark.parametrize("set_, g, s, d", [("factor4", 0, 5, 5), ("columns16", 0, 5, 17)])
def test_prefixes_up_to_d_take_no_covariance_step(host, set_, g, s, d):
    """n = d - 1, d, d + 1: no covariance step for n <= d, and a record without one is the diagonal predictive's"""
    diag_host, split_host = E.host_lib(), SP.host_lib()
    full = wide.draw_set(set_)
    for n in (d - 1, d, d + 1):
        gene = cases.gene_of(cases.prefix(full, n), g)
        for split in (False, True):
            got = X.host_cell(host, gene, s, k_threshold=0.1, split=split)
            print(set_, "n", n, "split", split, "iterations", got[11], "cov_iterations", got[12], "khat", got[9], "mean", got[0])
            if n <= d:
                assert got[12] == 0, (n, split)
            if got[12] != 0:
                continue
            dg = (SP.host_exact_cell(split_host, gene, s, k_threshold=0.1) if split else E.host_cell(diag_host, gene, s, k_threshold=0.1))
            tr = got[NH:NH + d * d].reshape(d, d)
            mine = np.concatenate([got[:12], np.diag(tr), got[NH + d * d:], got[13:14] if split else []])
            assert np.array_equal(np.isnan(mine), np.isnan(dg)) and np.array_equal(np.isinf(mine), np.isinf(dg)), (n, split, mine, dg)
            assert all(mine[i] == dg[i] or (np.isnan(mine[i]) and np.isnan(dg[i])) for i in (4, 5, 6, 7, 8, 11)), (n, split)
            assert max(X._err(a, b, i in (2, 3)) for i, (a, b) in enumerate(zip(mine, dg))) <= BOUND, (n, split)


FACTOR4_CHAINS, FACTOR4_BATCHES = 60000, 10


def held_out_predictive(chains=FACTOR4_CHAINS, batches=FACTOR4_BATCHES, seed=31):
    """the held-out predictive of the factor4 cell from `chains` independent chains of wide_design_cases.metropolis with the cell
    excluded (the seeds of tests/test_loo_mm_cov_host.py), reduced per batch with loo_mm_exact_restate.predictive under uniform
    weights: {statistic: (mean of the batch estimates, their standard deviation / sqrt(batches))} for mean, lower, upper and
    log p_ge"""
    from tests import loo_mm_cov_cases as cov_cases
    spec = wide.SPECS["factor4"]
    g, s = cov_cases.FACTOR4["g"], cov_cases.FACTOR4["s"]
    Xd = spec["X"]
    S_, Cc = Xd.shape
    y = np.asarray(spec["counts"], np.int32)[g]
    expo = np.linspace(-0.1, 0.1, S_)
    excl = np.zeros(S_, bool)
    excl[s] = True
    per = chains // batches
    est = {k: [] for k in ("mean", "lower", "upper", "log_p_ge")}
    for b in range(batches):
        T = wide.metropolis(np.random.default_rng([seed, b]), per, y, excl, expo, Xd, True)
        mu, phi = np.exp(expo[s] + Xd[s] @ T[:Cc]), np.exp(-T[Cc])
        p = E.predictive(np.full(per, 1.0 / per), mu, phi, int(y[s]), 0.025, 0.975)
        for k in ("mean", "lower", "upper"):
            est[k].append(p[k])
        est["log_p_ge"].append(np.log(p["p_ge"]))
    return {k: (float(np.mean(v)), float(np.std(v, ddof=1) / np.sqrt(batches))) for k, v in est.items()}


def test_factor4_cell(host):
    """for mean and for upper the distance to the held-out reference with the covariance candidate is at most half the distance
    without it, and the reference's batch scatter is under a quarter of the gap that decides this (half the distance without,
    less the distance with). Under the restatements: upper 572 without, 64 with, gap 222, scatter 1.2; mean 214, 34, 73, 0.23.
    lower, log p_ge and the split row are printed, not asserted (log p_ge only moves from 2.87 to 1.29 nats)."""
    gene = cases.gene_of(wide.draw_set("factor4"), 0)
    s = 5
    diag = E.host_cell(E.host_lib(), gene, s)
    got = X.host_cell(host, gene, s)
    sp = X.host_cell(host, gene, s, split=True)
    plain = X.host_cell(host, gene, s, max_iters=0)
    ref = held_out_predictive()
    for name, r in (("plain PSIS", plain), ("matching of ppcx_loo_mm.h", diag), ("with the covariance candidate", got), ("with it and split", sp)):
        print(name, "khat", r[9], "mean", r[0], "lower", r[4], "upper", r[5], "log p_ge", np.log(r[3]),
              "khat_split", r[13] if r.size == got.size else None)
    print("held-out reference (value, batch scatter)", ref)
    assert got[12] > 0 and got[9] < 0.7 <= diag[9]
    for k, i in (("mean", 0), ("upper", 5)):
        d_without, d_with = abs(diag[i] - ref[k][0]), abs(got[i] - ref[k][0])
        gap = 0.5 * d_without - d_with
        print(k, "distance without", d_without, "with", d_with, "gap", gap, "scatter", ref[k][1])
        assert ref[k][1] < 0.25 * gap, (k, ref[k][1], gap)
        assert d_with <= 0.5 * d_without, (k, d_with, d_without)
