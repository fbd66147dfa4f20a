"""The robot side of a step — collision per type, dmin, reward, done, info — on the oracle alone (no GPU).

Three things are asserted here, all about the INPUTS that tests/test_robot_outcome_gpu.py runs on the device:

1. The recipe that turns a row of tests/golden/collisions.npz or a point of tests/golden/grid.npz into one env of a batch
   gives the reference's recorded answer when the oracle takes the step (every row; every form of the step that the GPU
   test drives, with the oracle standing in for the device handle: the GPU test's bodies, dry-run).
2. The plain restatements written in tests/helpers.py (the grid window of simulator/env.py:227-271, the ordered walk of
   :303-313) equal the oracle on the constructed batches.
3. The constructed batches hold every case they were built for: the order-dependent cases of the per-type walk, every
   rung of the reward ladder and every contested pair of adjacent rungs, the three segments of time_reward with both
   equalities.  These are requirements on the builders: when one is missed, change the builder, not the condition.

Quarters: orca_step_kernel gives lane q of an env the humans [q * c, (q + 1) * c) with c = ceil(N / 4), so for some N
(5, 6, 9, ...) the last quarter holds nobody; "the first collider in every quarter" is asked of the quarters that
hold a human.

The tables go to profiles/robot_outcome_coverage.txt between its BEGIN / END markers."""
import os

import numpy as np
import pytest

from ebcsim import _abi
from ebcsim.scene import pack_grid
from oracle import oracle
from helpers import (_blank_batch, ARRIVALS, GRID_BORDER, GRID_MAPS, GRID_RADII, LADDER, LADDER_BORDER, ORDERED_COUNTS, OUTCOME_FORMS,
                     TIME_REWARD, TIME_STEPS, WIDE_RADIUS, check_against_oracle, check_golden_collisions,
                     check_obstacle_outcome, check_ordered, golden_grid_batches, grid_window_batches, ladder_batch,
                     ladder_params, load, oracle_env, ordered_coverage, outcome_params,
                     params_of, time_reward_batch, time_reward_forms, unicycle_batch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "robot_outcome_coverage.txt")
report = {}  # part -> lines of the table


def test_golden_collisions_recipe():
    """All 12008 rows: flag == coll, the other two dmin slots inf, min(dmin_in, dmin[type]) == dmin_out."""
    stats = check_golden_collisions(oracle_env, OUTCOME_FORMS)
    assert set(stats) == set(OUTCOME_FORMS)
    for form, (not_identical, rows, worst) in stats.items():
        assert rows == 9008 - 6 + sum(1 for k in range(6) if load("collisions")["kin"][k] == 0)
    report["1 golden collisions"] = ["envs: 12008 (one per row; handles per (kinematics, dt), the six unit rows on their own)",
                                     "oracle, every form: %d of %d holonomic rows not bit-identical, largest unicycle |diff| %.3g"
                                     % stats["step"]]


def test_golden_grid_recipe():
    """All 7200 points, the border rows as calls of their own."""
    total = hits = 0
    for k, (b, border, exp) in enumerate(golden_grid_batches()):
        assert b.n % 4
        check_obstacle_outcome(oracle_env, outcome_params(), b, border, exp, "golden grid, call %d" % k)
        total += b.n
        hits += int(exp.sum())
    assert total == 7200 and 0.05 < hits / total < 0.95
    report["2 golden grid"] = ["envs: %d in %d calls, %d collide" % (total, len(golden_grid_batches()), hits)]


@pytest.mark.parametrize("geometry", GRID_MAPS, ids=lambda g: "%gm-%gm" % g)
def test_grid_windows_restated(geometry):
    """The restatement equals the oracle's leaf and the oracle's step on every constructed window, and the windows are
    the ones asked for: more than eight rows, clipped to nothing, both outcomes of every border equality, and on the
    128-cell map a window over all 128 columns."""
    size, res = geometry
    G = int(round(size / res))
    lines = []
    for b, border, exp, notes, occs in grid_window_batches(size, res):
        assert b.n % 4
        params = outcome_params(map_size_m=size, map_resolution=res)
        rows, widths, clipped = [], [], 0
        for e in range(b.n):
            px, py, rad = b.robot[e, 0], b.robot[e, 1], b.robot[e, 4]
            got = oracle.grid_collision(b.grid[e], G, size, res, px, py, rad, border)
            assert got == bool(exp[e]), (notes[e], px, py, rad)
            np.testing.assert_array_equal(pack_grid(1.0 - occs[e].astype(np.float64)), b.grid[e])
            h = int(np.ceil(rad / np.sqrt(2.0) / res))
            ix, iy = int(round((px + size / 2) / res)), int(round((py + size / 2) / res))
            r = max(min(ix + h, G) - max(ix - h, 0), 0)
            w = max(min(iy + h, G) - max(iy - h, 0), 0)
            rows.append(r)
            widths.append(w)
            clipped += int(r == 0 or w == 0)
        check_obstacle_outcome(oracle_env, params, b, border, exp, "windows G %d" % G)
        if border is None:
            assert max(rows) > 8 and clipped > 0 and 0 < exp.sum() < b.n
            want_rows = [2 * int(np.ceil(r / np.sqrt(2.0) / res)) for r in GRID_RADII]
            assert res != 0.1 or want_rows == [10, 14, 22]
            for want in want_rows:
                assert want in rows, "no window of %d rows" % want
            if G == 128:
                wide = [e for e in range(b.n) if widths[e] == 128]
                assert wide and any(exp[e] for e in wide) and not all(exp[e] for e in wide)
                assert int(np.ceil(WIDE_RADIUS / np.sqrt(2.0) / res)) >= 64
        else:
            eq = [e for e in range(b.n) if notes[e] == "border equality"]
            ulp = [e for e in range(b.n) if notes[e] == "one ulp inside the border"]
            assert len(eq) >= 4 and exp[eq].all() and len(ulp) >= 4 and not exp[ulp].any()
            assert border == GRID_BORDER
        lines.append("G %3d %s: %d envs, %d collide, windows of up to %d rows x %d columns, %d clipped to nothing"
                     % (G, "border   " if border else "no border", b.n, int(exp.sum()), max(rows), max(widths), clipped))
    report["3 grid windows, G %3d" % G] = lines


@pytest.mark.parametrize("interleaved", [False, True], ids=["grouped", "interleaved"])
@pytest.mark.parametrize("N", ORDERED_COUNTS)
def test_ordered_reduction_restated(N, interleaved):
    """Restatement == oracle bit for bit (every form of the step, the oracle standing in), and the batch holds every
    order-dependent case."""
    b, _ = check_ordered(oracle_env, N, interleaved, OUTCOME_FORMS)
    assert b.n % 4 and b.n % 16 and b.n % 64
    if not interleaved:
        assert (np.diff(b.type.astype(int), axis=1)[np.arange(b.N - 1)[None] < b.n_humans[:, None] - 1] >= 0).all()
    cov = ordered_coverage(b)
    assert cov["empty env"] >= 1
    if N >= 5:
        c = -(-N // 4)
        for t in range(3):
            for q in range(4):
                if q * c < N:
                    assert cov["type %d first collider in quarter %d" % (t, q)] >= 1, (N, t, q)
            for k in ("closer_behind", "closer_before_earlier_quarter", "second_collider", "without a member"):
                assert cov["type %d %s" % (t, k)] >= 1, (N, t, k)
        for k in ("two types collide", "three types collide", "humans but no collider"):
            assert cov[k] >= 1, (N, k)
    q = lambda t: "/".join(str(cov["type %d first collider in quarter %d" % (t, k)]) for k in range(4))  # noqa: E731
    s = lambda k: "/".join(str(cov["type %d %s" % (t, k)]) for t in range(3))  # noqa: E731
    report.setdefault("4 ordered reduction", [
        "envs per batch: %d; per type adult/bicycle/child; first collider per quarter q0/q1/q2/q3" % b.n,
        "%-16s %-11s %-11s %-11s %-9s %-9s %-9s %-9s %5s %5s %5s %5s" % (
            "batch", "first(ad)", "first(bi)", "first(ch)", "behind", "before", "second", "nomember", "2coll", "3coll",
            "none", "empty")])
    report["4 ordered reduction"].append("%-16s %-11s %-11s %-11s %-9s %-9s %-9s %-9s %5d %5d %5d %5d" % (
        "N %2d %s" % (N, "interleaved" if interleaved else "grouped"), q(0), q(1), q(2), s("closer_behind"),
        s("closer_before_earlier_quarter"), s("second_collider"), s("without a member"), cov["two types collide"],
        cov["three types collide"], cov["humans but no collider"], cov["empty env"]))


RUNGS = ("timeout", "child", "bicycle", "adult", "obstacle", "goal", "danger child", "danger bicycle", "danger adult",
         "rotation", "nothing")


def _conditions(params, b, act, border, out):
    """Per env, which rungs' conditions hold (read from the oracle's outputs and its grid leaf; the time and the
    turn from the inputs) and which rung the oracle took."""
    G = 90
    dd, f = list(params.discomfort_dist), list(params.discomfort_factor)
    conds, taken = [], []
    for e in range(b.n):
        dm = out["dmin"][e]
        wall = oracle.grid_collision(None if b.grid is None else b.grid[e], G, params.map_size_m, params.map_resolution,
                                     b.robot[e, 0], b.robot[e, 1], b.robot[e, 4], border)
        c = {"timeout": 0.0 >= params.time_limit,
             "child": np.isinf(dm[2]), "bicycle": np.isinf(dm[1]), "adult": np.isinf(dm[0]),  # a member, and no distance
             "obstacle": wall, "goal": out["dist_to_goal"][e] < b.robot[e, 4],
             "danger child": dm[2] < dd[2], "danger bicycle": dm[1] < dd[1], "danger adult": dm[0] < dd[0],
             "rotation": params.robot_kinematics != _abi.HOLONOMIC and abs(act[e, 1]) > 0 and params.rotation_penalty_factor != 0,
             "nothing": True}
        info, r = int(out["info"][e]), float(out["reward"][e])
        by_info = {_abi.INFO_TIMEOUT: "timeout", _abi.INFO_COLLISION_CHILD: "child", _abi.INFO_COLLISION_BICYCLE: "bicycle",
                   _abi.INFO_COLLISION_ADULT: "adult", _abi.INFO_COLLISION_OBSTACLE: "obstacle", _abi.INFO_REACH_GOAL: "goal"}
        if info in by_info:
            rung = by_info[info]
        elif info == _abi.INFO_DANGER:
            fits = [t for t in (2, 1, 0) if c[("danger adult", "danger bicycle", "danger child")[t]]
                    and r == (dm[t] - dd[t]) * f[t] * params.time_step]
            assert fits, (e, r)
            rung = ("danger adult", "danger bicycle", "danger child")[fits[0]]
        else:
            rung = "rotation" if r != 0 else "nothing"
        assert c[rung] and bool(out["done"][e]) == (rung in RUNGS[:6]), (e, rung)
        assert rung == next(k for k in RUNGS if c[k]), (e, rung)  # the ladder's order
        conds.append(c)
        taken.append(rung)
    return conds, taken


def test_reward_ladder_coverage():
    """Every rung taken, under either reward form; every pair of adjacent rungs contested with the higher one winning;
    the exact thresholds fall on the side the reference puts them."""
    taken_all, contested = {}, set()
    runs = []
    for new_reward in (0, 1):
        for wall, border in (("grid", None), ("border", LADDER_BORDER)):
            for limit in (25.0, 0.0):
                runs.append((ladder_params(new_reward, limit), ladder_batch(wall), None, border))
    for factor in (0.0, 0.5):
        ub, uact = unicycle_batch()
        runs.append((ladder_params(0, kinematics=_abi.UNICYCLE, rotation_penalty_factor=factor), ub, uact, None))
    envs = 0
    for params, b, act, border in runs:
        assert b.n % 4
        act = np.zeros((b.n, 2)) if act is None else act
        ref, _ = check_against_oracle(oracle_env, params, b, act, border, "ladder")  # the forms, dry-run on the oracle
        conds, taken = _conditions(params, b, act, border, ref)
        envs += b.n
        for e, (c, rung) in enumerate(zip(conds, taken)):
            taken_all[(rung, params.new_reward)] = taken_all.get((rung, params.new_reward), 0) + 1
            k = RUNGS.index(rung)
            if k + 1 < len(RUNGS) and c[RUNGS[k + 1]]:
                contested.add((rung, RUNGS[k + 1]))
        if params.time_limit == 0:
            assert (ref["info"] == _abi.INFO_TIMEOUT).all()
            goal_term = 1 - ref["dist_to_goal"] / params.max_goal_distance
            np.testing.assert_array_equal(ref["reward"], goal_term if params.new_reward else np.zeros(b.n))
        elif params.robot_kinematics == _abi.HOLONOMIC and border is None:
            m = dict((name, e) for e, name in enumerate(b.meta) if isinstance(name, str))
            assert taken[m["goal at the radius"]] == "nothing" and taken[m["goal one ulp inside"]] == "goal"
            first = b.meta.index("gap == discomfort_dist")
            assert taken[first:first + 3] == ["nothing"] * 3
            assert taken[first + 3:first + 6] == ["danger adult", "danger bicycle", "danger child"]
            assert taken[first + 6:first + 9] == ["danger adult", "danger bicycle", "danger child"]  # gap 0: no collision
            assert (ref["dmin"][first + 6:first + 9][np.eye(3, dtype=bool)] == 0).all()
    for rung in RUNGS:
        for new_reward in (0, 1) if rung != "rotation" else (0,):
            assert taken_all.get((rung, new_reward)), "rung %s (new_reward %d) never taken" % (rung, new_reward)
    for pair in zip(RUNGS[:-1], RUNGS[1:]):
        assert pair in contested, "rungs %s / %s never contested" % pair
    assert len(set(LADDER["collision_penalty"])) == 4 and len(set(LADDER["discomfort_factor"])) == 3
    report["5 reward ladder"] = ["envs: %d in %d calls (267 per ladder batch: grid / border wall x new_reward 0 / 1 x "
                                 "time_limit 25 / 0; 9 per unicycle batch)" % (envs, len(runs)),
                                 "rung taken (new_reward 0 / 1): " + ", ".join(
                                     "%s %d/%d" % (r, taken_all.get((r, 0), 0), taken_all.get((r, 1), 0)) for r in RUNGS),
                                 "adjacent rungs contested: %d of %d" % (len(contested & set(zip(RUNGS[:-1], RUNGS[1:]))),
                                                                         len(RUNGS) - 1)]


def test_time_reward_coverage():
    """The three segments of time_reward and both closed ends of the middle one occur, and the robot that never arrives
    times out in the step that starts at t == time_limit."""
    b, params = time_reward_batch()
    res = time_reward_forms(oracle_env)
    o = res["step"]
    for form in res:
        for k in o:
            assert res[form][k].tobytes() == o[k].tobytes()
    assert b.n % 4 and o["info"].shape == (TIME_STEPS, b.n)
    segments = set()
    for e, t in enumerate(ARRIVALS):
        k = int(np.argmax(o["done"][:, e]))  # the first terminal step
        if t is None:
            assert o["info"][k, e] == _abi.INFO_TIMEOUT and k * params.time_step == params.time_limit and k == TIME_STEPS - 1
            continue
        assert o["info"][k, e] == _abi.INFO_REACH_GOAL and k * params.time_step == t, (e, k)
        bonus = o["reward"][k, e] - (1 - o["dist_to_goal"][k, e] / params.max_goal_distance)
        seg = "before" if t < params.time_good else ("middle" if t <= params.time_max else "after")
        want = {"before": 1.0, "after": 0.0}.get(seg, (params.time_max - t) / (params.time_max - params.time_good))
        assert abs(bonus - want) <= 1e-12, (t, bonus, want)
        segments.add(seg + (" ==" if t in (params.time_good, params.time_max) else ""))
    assert segments == {"before", "middle", "middle ==", "after"} and TIME_REWARD["time_good"] in ARRIVALS and TIME_REWARD["time_max"] in ARRIVALS
    report["5 time_reward"] = ["envs: %d, %d steps; arrivals at t = %s; segments %s" % (
        b.n, TIME_STEPS, ", ".join("never" if t is None else "%g" % t for t in ARRIVALS), ", ".join(sorted(segments)))]


def test_reward_golden_rows_through_a_step():
    """reward.npz rows whose ladder inputs can be read off and realised by a step: dmin all inf and no collision recorded
    is an env with no human and no map; the recorded time goes into the oracle's state.  The step reproduces the
    recorded reward, done, info and dist_to_goal."""
    z = load("reward")
    used = 0
    kinds = set()
    for ci in range(int(z["n_configs"])):
        params = params_of(z, "params_%d" % ci)
        rin, rout = z["in_%d" % ci], z["out_%d" % ci]
        sel = np.nonzero(np.isinf(rin[:, 12:15]).all(1) & (rin[:, 15:19] == 0).all(1))[0]
        if not len(sel):
            continue
        b = _blank_batch(len(sel), 1, 0)
        b.n_humans[:] = 0
        b.robot[:] = rin[sel, :9]
        env = oracle_env(params, b.n, 1, 0)
        env.reset(b)
        env.a["global_time"][:] = rin[sel, 11]
        out = env.step(robot_action=rin[sel, 9:11], human_policy=_abi.HUMAN_LINEAR)
        exp = rout[sel]
        np.testing.assert_array_equal(out["info"], exp[:, 2].astype(np.uint8))
        np.testing.assert_array_equal(out["done"].astype(bool), exp[:, 1].astype(bool))
        np.testing.assert_allclose(out["reward"], exp[:, 0], atol=1e-12, rtol=0, equal_nan=True)
        ok = ~np.isnan(exp[:, 3])
        np.testing.assert_allclose(out["dist_to_goal"][ok], exp[ok, 3], atol=1e-12, rtol=0)
        used += len(sel)
        kinds.update(out["info"].tolist())
    assert used > 100 and {_abi.INFO_NOTHING, _abi.INFO_REACH_GOAL, _abi.INFO_TIMEOUT} <= kinds
    report["5 reward.npz"] = ["%d rows with no human in range replayed through a step" % used]


BEGIN, END = "# BEGIN generated by tests/test_robot_outcome_cpu.py", "# END generated"


def test_write_the_coverage_table():
    """Runs last in this module: the tables of the tests above, between the markers of the profile."""
    if not {"1 golden collisions", "2 golden grid", "4 ordered reduction", "5 reward ladder"} <= set(report):
        return  # a selection of this module's tests ran: nothing to record
    lines = [BEGIN]
    for part in sorted(report):
        lines.append("## part " + part)
        lines += ["  " + ln for ln in report[part]]
    lines.append(END)
    new = "\n".join(lines) + "\n"
    old = open(TABLE).read() if os.path.exists(TABLE) else ""
    if BEGIN in old and END in old:
        text = old[:old.index(BEGIN)] + new + old[old.index(END) + len(END) + 1:]
    else:
        text = old + new
    if text != old:
        with open(TABLE, "w") as f:
            f.write(text)
