"""What tests/test_robot_orca_wide_gpu.py relies on, asserted on the oracle alone (no GPU).

Above 64 rows the GPU test has no oracle for the full batch and checks the kernel against the oracle on the REDUCED batch
(orca_wide_cases.reduced_batch: the env of the selected rows).  Here (1) that reduction is shown to be exact on the oracle
for every batch of at most 64 rows the GPU test uses, (2) the batches are shown to cover what a selection kernel can get
wrong — more rows in range than max_neighbors, selected rows in every 32-row tile, a selection wholly behind row 32,
ragged envs with 0, 1 and at most 32 rows inside a wide handle —, (3) the traced oracle shows that envs with more than 32
rows reach every branch of RVO2, and (4) the hand-built ties decide between two rows in different tiles.

The conditions are requirements on the batches: when one is missed, change the batch, not the condition."""
import numpy as np
import pytest

from helpers import batch_rows, orca_case_params
from oracle import oracle
from orca_wide_cases import (ORACLE_CASES, ORACLE_RUNS, PARAM_SETS, REDUCED_CASES, SAFETIES, TIES_ROWS, TILE, full_reference,
                             oracle_robot_orca, reduced_batch, reduced_reference, rows_of, select, ties_batch, wide_batch)


def _same(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(-1))
    assert not len(bad), "%s: %d of %d envs differ, the first %d: %r / %r" % (tag, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]])


@pytest.mark.parametrize("safety", SAFETIES)
@pytest.mark.parametrize("case,ps", ORACLE_RUNS, ids=lambda v: v if isinstance(v, str) else "N%d-S%d" % v)
def test_reduction_is_exact_on_the_oracle(case, ps, safety):
    N, S = case
    full = oracle_robot_orca(wide_batch(N, S), orca_case_params(0, ps), safety) if ps == "all" else full_reference(N, S, ps, safety)
    assert np.isfinite(full).all()
    _same(full, reduced_reference(case, wide_batch(N, S), ps, safety), "N %d S %d %s safety %g" % (N, S, ps, safety))


@pytest.mark.parametrize("safety", SAFETIES)
def test_reduction_is_exact_on_the_ties(safety):
    b, params = ties_batch(40), orca_case_params(0, "default")
    _same(oracle_robot_orca(b, params, safety), reduced_reference(("ties", 40), b, "default", safety), "ties safety %g" % safety)


@pytest.mark.parametrize("case", ORACLE_CASES + REDUCED_CASES, ids=lambda c: "N%d-S%d" % c)
def test_batches_cover_the_selection(case):
    N, S = case
    R = N + S
    b = wide_batch(N, S)
    assert b.n % 2 == 1  # the last workgroup of a launch is half filled
    rows = b.n_humans + b.n_static
    assert int((rows > TILE).sum()) > b.n // 2
    f = b.forced
    assert rows[f["none"]] == 0 and rows[f["one"]] == 1 and 1 < rows[f["narrow"]] <= TILE
    assert b.n_humans[f["static_only"]] == 0 and b.n_static[f["static_only"]] == S and b.n_static[f["humans_only"]] == 0
    assert len(set(rows.tolist())) > 10  # ragged
    for ps in PARAM_SETS:
        params = orca_case_params(0, ps)
        sel = select(b, params)
        tiles, crowded = set(), 0
        for e in range(b.n):
            _, idx = rows_of(b, e)
            chosen = idx[sel[e][0]]
            tiles |= set((chosen // TILE).tolist())
            crowded += int(rows[e] > TILE and sel[e][1] > max(params.orca_max_neighbors, 10))
        assert crowded >= 10, (ps, crowded)
        assert tiles == set(range((R + TILE - 1) // TILE)), (ps, tiles)
    # the env whose first 32 rows stand out of range: a selection wholly behind them, and not an empty one
    _, idx = rows_of(b, f["behind"])
    chosen = idx[select(b, orca_case_params(0, "default"))[f["behind"]][0]]
    assert len(chosen) == min(R - TILE, 10) and (chosen >= TILE).all(), chosen


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    return oracle.Traced(str(tmp_path_factory.mktemp("oracle_trace_wide")))


@pytest.mark.parametrize("case", ORACLE_CASES + REDUCED_CASES, ids=lambda c: "N%d-S%d" % c)
def test_wide_envs_reach_every_branch(traced, case):
    """The envs with more than 32 rows alone, on the traced oracle (above 64 rows: their reduced envs, which take the same
    branches): cut-off circle, both legs, colliding, a linearProgram2 failure, linearProgram3 with projected lines."""
    N, S = case
    b = wide_batch(N, S)
    params = orca_case_params(0, "default")
    wide = batch_rows(b, np.flatnonzero(b.n_humans + b.n_static > TILE))
    pooled = {}
    for safety in SAFETIES:
        traced.reset()
        run = wide if N + S <= 64 else reduced_batch(wide, params)
        got = oracle_robot_orca(run, params, safety, library=traced.lib)
        assert np.isfinite(got).all()
        for k, v in traced.counts().items():
            pooled[k] = pooled.get(k, 0) + v
    assert pooled["agents"] == 2 * wide.n
    for k in ("line_circle", "line_left_leg", "line_right_leg", "line_colliding", "lp3_entered", "lp3_bodies"):
        assert pooled[k] >= 1, (k, pooled)
    assert N + S > 64 or pooled["nb_truncated"] >= 1, pooled  # a reduced env has nothing left to drop
    assert pooled["lp2_fail_at_0"] + pooled["lp2_fail_at_1"] + pooled["lp2_fail_at_2"] + pooled["lp2_fail_at_3_or_more"] >= 1, pooled
    # a failure at line 1 or later: linearProgram3 projects the lines before it
    assert pooled["lp2_fail_at_1"] + pooled["lp2_fail_at_2"] + pooled["lp2_fail_at_3_or_more"] >= 1, pooled


@pytest.mark.parametrize("R", TIES_ROWS)
def test_ties_go_to_the_lower_row(R):
    """Equal float32 distSq at ranks 9 and 10, the two rows in different 32-row tiles: the numpy selection takes the
    lower index, drops the other, and the answer depends on which one it is."""
    b = ties_batch(R)
    params = orca_case_params(0, "default")
    sel = select(b, params)
    f = np.float32
    straddle = set()
    for e, (lo, hi) in enumerate(b.pairs):
        rows, idx = rows_of(b, e)
        assert len(idx) == R
        d = (f(0) - rows[:, 0].astype(f)) ** 2 + (f(0) - rows[:, 1].astype(f)) ** 2
        assert d[lo] == d[hi] and int((d < d[lo]).sum()) == 9 and int((d == d[lo]).sum()) == 2
        assert sel[e][1] == R  # every row in range
        chosen = set(idx[sel[e][0]].tolist())
        assert len(chosen) == 10 and lo in chosen and hi not in chosen, (e, lo, hi, sorted(chosen))
        assert lo // TILE != hi // TILE
        straddle |= {t for t in (1, 2, 3) if lo < t * TILE <= hi}
    assert straddle >= ({1} if R <= 64 else {1, 2})
    # the other choice is another answer: swap the pair's rows and the oracle's reduced solve moves
    swapped = ties_batch(R)
    swapped = batch_rows(swapped, np.arange(swapped.n))
    for e, (lo, hi) in enumerate(b.pairs):
        for (k, n0) in (("px", "spx"), ("py", "spy")):
            def cell(r):
                return (getattr(swapped, k), r) if r < b.N else (getattr(swapped, n0), r - b.N)
            (a, i), (c, j) = cell(lo), cell(hi)
            a[e, i], c[e, j] = c[e, j], a[e, i]
    moved = oracle_robot_orca(reduced_batch(swapped, params), params, 0.0)
    kept = reduced_reference(("ties", R), b, "default", 0.0)
    assert (moved.view(np.uint64) != kept.view(np.uint64)).any(-1).sum() >= len(b.pairs) // 2
