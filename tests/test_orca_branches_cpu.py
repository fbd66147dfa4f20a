"""Which branches of RVO2 the ORCA batches of tests/helpers.py reach: a property of the INPUTS, asserted from the oracle
alone (no GPU).  The oracle compiled with -DORC_TRACE (oracle.Traced: a second shared object, built here into a
temporary directory) counts every branch of computeNeighbors / computeNewVelocity / linearProgram1-3 it takes over exactly
the batches, parameter sets and steps that tests/test_orca_branches_gpu.py runs on the device.  The conditions below are
requirements on the generators: when one is missed, change a seed or an env count in helpers.py, not the condition.

Two conditions cannot hold at the smallest counts and are asked from where they can: a human alone (N = 1) has no
ORCA line at all (asserted: every agent there has zero neighbours), and an exact distance tie needs two others (N >= 3,
or N = 2 with a visible robot).

The sets that move time_step, orca_time_horizon and orca_safety_space off the values of every golden (0.25, 5, 0) are
asked two more things: that at least a tenth of the humans get another first velocity than under the default set (else a
kernel that ignored the field would go unnoticed), and that the colliding branch (invTimeStep) and the cut-off circle and
both legs (invTimeHorizon) are still reached.

The table of counts goes to profiles/orca_branch_coverage.txt between its BEGIN / END markers."""
import os

import numpy as np
import pytest

from helpers import (ORCA_HUMAN_CASES, ORCA_HUMAN_COUNTS, ORCA_MOVED_SETS, ORCA_PARAM_SETS, ORCA_ROBOT_CASES,
                     ORCA_ROBOT_MOVED_CASES, ORCA_STEPS, orca_case_id, orca_case_params, orca_human_batch, orca_reference,
                     orca_robot_batch, orca_robot_case_id, orca_robot_reference)
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "orca_branch_coverage.txt")
SAFETIES = (0.0, 0.15)


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    return oracle.Traced(str(tmp_path_factory.mktemp("oracle_trace")))


def _pool(a, b):
    return {k: max(a.get(k, 0), v) if k == "lp3_most_bodies" else a.get(k, 0) + v for k, v in b.items()}


def _ties_and_nan_inputs(b, rv, neighbor_dist):
    """From the reset scene alone, in the float32 arithmetic of Agent::insertAgentNeighbor: agents with two in-range
    others at exactly the same squared distance, and pairs with equal position and velocity (w = 0: a NaN line)."""
    ties = twins = 0
    f = np.float32
    for e in range(b.n):
        n = int(b.n_humans[e])
        pos = np.stack([b.px[e, :n], b.py[e, :n]], 1).astype(f)
        vel = np.stack([b.vx[e, :n], b.vy[e, :n]], 1).astype(f)
        if rv:
            pos = np.concatenate([pos, b.robot[e, None, 0:2].astype(f)])
            vel = np.concatenate([vel, b.robot[e, None, 2:4].astype(f)])
        for i in range(n):
            others = [k for k in range(len(pos)) if k != i]
            d = pos[i] - pos[others]
            dist = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]  # float32, one rounding per operation
            dist = dist[dist < f(neighbor_dist) * f(neighbor_dist)]
            ties += int(len(np.unique(dist)) < len(dist))
            twins += int(((pos[others] == pos[i]).all(1) & (vel[others] == vel[i]).all(1)).any())
    return ties, twins


@pytest.fixture(scope="module")
def coverage(traced):
    """{case: counts} over every human case and {(N, S): counts} over every robot case, with the bit-identity of the
    traced build and the finiteness of every output checked on the way."""
    human, robot = {}, {}
    for case in ORCA_HUMAN_CASES:
        N, rv, ps = case
        plain = orca_reference(case)
        traced.reset()
        tr = orca_reference(case, library=traced.lib)
        c = traced.counts()
        for t in range(ORCA_STEPS):
            for k, v in plain["out"][t].items():
                assert v.tobytes() == tr["out"][t][k].tobytes(), (case, t, k)
                assert np.isfinite(v).all() or k == "dmin", (case, t, k)  # dmin is +inf where a class has no human
            for k, v in plain["state"][t].items():
                assert v.tobytes() == tr["state"][t][k].tobytes(), (case, t, k)
                assert np.isfinite(v).all(), (case, t, k)
        c["tie_agents"], c["twin_agents"] = _ties_and_nan_inputs(orca_human_batch(N, rv), rv,
                                                                 orca_case_params(rv, ps).orca_neighbor_dist)
        human[case] = c
    for case in ORCA_ROBOT_CASES + ORCA_ROBOT_MOVED_CASES:
        pooled = {}
        for safety in SAFETIES:
            plain = orca_robot_reference(case, safety)
            traced.reset()
            tr = orca_robot_reference(case, safety, library=traced.lib)
            assert plain.tobytes() == tr.tobytes(), (case, safety)
            assert np.isfinite(plain).all(), (case, safety)
            pooled = _pool(pooled, traced.counts())
        robot[case] = pooled
    return human, robot


def _others(N, rv):
    return N - 1 + rv


@pytest.mark.parametrize("N,rv", ORCA_HUMAN_COUNTS)
def test_every_human_count_reaches_the_branches(coverage, N, rv):
    c = coverage[0][N, rv, "default"]
    others = _others(N, rv)
    if others == 0:
        assert c["nb_none"] == c["agents"] > 0
        return
    for k in ("line_colliding", "line_circle", "line_left_leg", "line_right_leg", "lp1_dir0", "lp3_entered"):
        assert c[k] >= 1, (k, c)
    if others >= 2:
        assert c["tie_agents"] >= 1, c
    if others >= 7:
        for k in ("lp1_fail_discriminant", "lp1_fail_parallel", "lp1_fail_interval", "lp1_dir1", "lp3_parallel_opposite",
                  "lp1_parallel_skip", "lp2_fail_at_3_or_more", "line_nan"):
            assert c[k] >= 1, (k, c)
        assert c["lp3_most_bodies"] >= 2, c
        assert c["twin_agents"] >= 1, c
    if others > 10:
        assert c["nb_truncated"] >= 1, c


@pytest.mark.parametrize("case", [c for c in ORCA_HUMAN_CASES if ORCA_PARAM_SETS[c[2]][:2] != (10, 10.0)], ids=orca_case_id)
def test_parameter_sets_truncate_and_leave_agents_alone(coverage, case):
    N, rv, ps = case
    c = coverage[0][case]
    if ps == "mn0":  # maxNeighbors 0: nobody has a neighbour, every in-range other is dropped
        assert c["nb_none"] == c["agents"] and c["nb_truncated"] >= 1 and c["lp1_dir0"] == 0, c
        return
    max_neighbors, neighbor_dist = ORCA_PARAM_SETS[ps][:2]
    if _others(N, rv) > max_neighbors:
        assert c["nb_truncated"] >= 1, c
    if neighbor_dist == 2.0:
        if _others(N, rv) >= 1:
            assert c["nb_out_of_range"] >= 1, c
        assert c["nb_none"] >= 1, c


def test_inner_lp2_failure_inside_lp3_occurs_somewhere(coverage):
    assert sum(c["lp3_inner_fail"] for c in coverage[0].values()) >= 1


def _changed_share(a, b, exists):
    """The share of existing humans whose velocity (either component) differs bitwise between two runs."""
    differ = (a.view(np.uint64) != b.view(np.uint64)).any(-1)
    return int((differ & exists).sum()), int(exists.sum())


@pytest.mark.parametrize("case", [c for c in ORCA_HUMAN_CASES if c[2] in ORCA_MOVED_SETS], ids=orca_case_id)
def test_moved_fields_are_seen_and_keep_the_branches(coverage, case):
    """time_step, the horizon and the humans' safety space off their defaults.  (a) At step 0 at least a tenth of the
    existing humans get another ORCA velocity than under "default", bit for bit: a kernel that ignored the field would
    differ from the oracle on as many.  (b) The case still reaches the colliding branch (invTimeStep) and (c) the cut-off
    circle and both legs (invTimeHorizon)."""
    N, rv, ps = case
    b = orca_human_batch(N, rv)
    exists = np.arange(N)[None, :] < b.n_humans[:, None]
    changed, total = _changed_share(orca_reference(case)["out"][0]["human_action"],
                                    orca_reference((N, rv, "default"))["out"][0]["human_action"], exists)
    assert 10 * changed >= total > 0, (changed, total)
    c = coverage[0][case]
    for k in ("line_colliding", "line_circle", "line_left_leg", "line_right_leg"):
        assert c[k] >= 1, (k, c)


@pytest.mark.parametrize("case", ORCA_ROBOT_MOVED_CASES, ids=orca_robot_case_id)
@pytest.mark.parametrize("safety", SAFETIES)
def test_robot_solve_takes_its_own_safety_space(case, safety):
    """The handle's safety space is the humans': under "saf0.1" the robot's solve is the default handle's, bit for bit,
    at either robot safety space; 0.15 in place of 0 moves it, and so does "all" (time step and horizon)."""
    plain = orca_robot_reference(case[:2], safety)
    moved = orca_robot_reference(case, safety)
    if case[2] == "saf0.1":
        assert moved.tobytes() == plain.tobytes()
    else:
        changed, total = _changed_share(moved, plain, np.ones(len(plain), bool))
        assert 10 * changed >= total, (changed, total)
    changed, total = _changed_share(moved, orca_robot_reference(case, SAFETIES[1] - safety), np.ones(len(plain), bool))
    assert 10 * changed >= total, (changed, total)


@pytest.mark.parametrize("case", ORCA_ROBOT_CASES + ORCA_ROBOT_MOVED_CASES, ids=orca_robot_case_id)
def test_robot_cases_collide_and_enter_lp3(coverage, case):
    c = coverage[1][case]
    assert c["agents"] == 2 * orca_robot_batch(*case[:2]).n  # the robot of every env, once per safety space
    assert c["line_colliding"] >= 1 and c["lp3_entered"] >= 1, c


def test_lp3_parallel_same_direction_by_hand(traced):
    """linearProgram3's "parallel, same direction: skip" (rare: the generated batches reach it a few times per case, see the
    table, and none is required to).  Hand-built: two others straight ahead on one ray, slower than the cut-off circle, give
    two cut-off lines with one and the same direction, the nearer one the looser; two others just overlapping the agent from
    the left and the right make linearProgram2 fail at line 1, so linearProgram3 walks lines 1, 2, 3 and meets the pair."""
    traced.reset()
    pos = np.array([[0, 0], [0.55, 0], [-0.55, 0], [0, 1.5], [0, 3.0]], np.float32)
    vel = np.array([[0, 0.1], [0, 0], [0, 0], [0, 0.3], [0, -0.3]], np.float32)
    radius = np.full(5, 0.3, np.float32)
    args = (0.25, 10.0, 10, 5.0, pos, vel, radius, 1.0, np.array([0, 1.0], np.float32))
    out = oracle.rvo2_agent0(*args, library=traced.lib)
    assert np.isfinite(out).all() and out == oracle.rvo2_agent0(*args)
    c = traced.counts()
    assert c["lp2_fail_at_1"] == 1 and c["lp3_bodies"] == 3 and c["lp3_parallel_same"] == 1, c
    test_lp3_parallel_same_direction_by_hand.count = c["lp3_parallel_same"]


COLUMNS = ("agents", "line_colliding", "line_circle", "line_left_leg", "line_right_leg", "line_nan", "tie_agents",
           "twin_agents", "nb_truncated", "nb_out_of_range", "nb_none", "lp1_dir0", "lp1_dir1", "lp1_fail_discriminant",
           "lp1_fail_parallel", "lp1_fail_interval", "lp1_parallel_skip", "lp2_fail_at_0", "lp2_fail_at_1",
           "lp2_fail_at_2", "lp2_fail_at_3_or_more", "lp3_entered", "lp3_bodies", "lp3_most_bodies", "lp3_parallel_same",
           "lp3_parallel_opposite", "lp3_inner_fail")
BEGIN, END = "# BEGIN generated by tests/test_orca_branches_cpu.py", "# END generated"


def test_write_the_coverage_table(coverage, traced):
    """branch x case, as counted above, into profiles/orca_branch_coverage.txt (between the markers; what else the file
    records stays).  Written only when it differs, so a run on an unchanged tree leaves the tree unchanged."""
    human, robot = coverage
    if not hasattr(test_lp3_parallel_same_direction_by_hand, "count"):
        test_lp3_parallel_same_direction_by_hand(traced)
    cases = [(orca_case_id(k), v) for k, v in human.items()] + [("robot " + orca_robot_case_id(k), v) for k, v in robot.items()]
    short = [c.replace("line_", "ln_").replace("_fail_", "_f_").replace("discriminant", "disc").replace("parallel", "par")
             .replace("interval", "intv").replace("_or_more", "+").replace("opposite", "opp").replace("out_of_range", "far")
             .replace("truncated", "trunc").replace("colliding", "coll").replace("entered", "in") for c in COLUMNS]
    lines = [BEGIN,
             "# one row per case: humans = %d steps from reset, every human of every env; robot = one call per env," % ORCA_STEPS,
             "# safety space 0 and 0.15 pooled.  Counts are sums over agents, lp3_most_bodies is the most on one agent;",
             "# tie_agents / twin_agents are counted from the reset scene (exact distSq ties; equal position and velocity).",
             "%-18s " % "case" + " ".join("%*s" % (max(len(h), 5), h) for h in short)]
    for name, v in cases:
        lines.append("%-18s " % name + " ".join("%*s" % (max(len(h), 5), v.get(c, "-")) for c, h in zip(COLUMNS, short)))
    lines.append("lp3_parallel_same, hand-built case (test_lp3_parallel_same_direction_by_hand): %d"
                 % test_lp3_parallel_same_direction_by_hand.count)
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
    assert all(h in text for h in short)
