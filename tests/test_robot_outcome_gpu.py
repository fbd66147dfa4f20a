"""The robot side of a step on the device (-m gpu): did the robot hit an adult, a bicycle, a child or a wall, how close
did it come to each type, and which reward, done and info follow.

Four kernels restate that reduction around the shared leaves of csrc/ebc_device.h (closest_dist, grid_collision,
reward_compute), and every batch here goes through all four where the form admits it (helpers.robot_outcome_forms):
step(HUMAN_LINEAR) is step_kernel, step(HUMAN_ORCA) orca_step_kernel's ENV role, lookahead(want_rows=False)
lookahead_kernel (chunks of 127 envs with the chunk's own 127 actions, the diagonal compared), and
step_k(FLAG_ONE_LAUNCH) rollout_kernel, which takes no border.  reward, done, info and dmin of the forms must agree
byte for byte, beside the bars each test holds them to.

1. every row of tests/golden/collisions.npz and 2. every point of tests/golden/grid.npz as one env: the reference's own
   recorded answers, which until now only the oracle was held to;
3. grid windows the goldens do not reach (more than the eight unrolled rows, three map geometries, cells on the 64-bit
   seam and the map's edges, windows clipped to nothing, the border's equalities, a window over all 128 columns)
   against a plain restatement and the oracle;
4. the ordered per-type walk (stop at the first hit, nothing behind it counts) at exact distances, bit for bit against
   a plain walk and the oracle, for grouped and for interleaved types;
5. the reward ladder over the cross product of its conditions, at its exact thresholds, with time_limit 0, over the
   three segments of time_reward, and for the unicycle's rotation penalty;
6. the device-output forms between canaries.

tests/test_robot_outcome_cpu.py asserts that these batches hold the cases they were built for.  Batch sizes are no
multiple of 4 (hence of no envs-per-wave count), so every launch ends in a part-filled wave."""
import numpy as np
import pytest

from ebcsim import _abi
from helpers import (ARRIVALS, GRID_MAPS, LADDER_BORDER, ORDERED_COUNTS, OUTCOME_FORMS, OUTCOME_KEYS, TIME_STEPS, Guarded,
                     assert_outcome, check_against_oracle, check_golden_collisions, check_obstacle_outcome, check_ordered,
                     golden_grid_batches, grid_window_batches, ladder_batch, ladder_params, oracle_env, oracle_outcome,
                     ordered_batch, outcome_params, time_reward_forms, unicycle_batch)
from test_gpu_parity import _env

pytestmark = pytest.mark.gpu


def test_golden_collisions():
    """All 12008 rows, human type = row index % 3: the collision flag read from info equals `coll`, the other two dmin
    slots are inf, min(dmin_in, dmin[type]) equals dmin_out at 1e-12 on the holonomic rows (at most 2 % of them not
    bit-identical: the bar and the cap tests/test_oracle_golden.py holds the oracle to) and at 1e-9 on the unicycle
    rows (cos / sin), and the reference's six known answers come out.  The counts are printed (-s)."""
    stats = check_golden_collisions(_env, OUTCOME_FORMS)
    assert set(stats) == set(OUTCOME_FORMS)


def test_golden_grid():
    """All 7200 points: INFO_COLLISION_OBSTACLE exactly where coll_k says so, a non-terminal INFO_NOTHING elsewhere; the
    rows that used the fixture's border as calls of their own (three forms)."""
    total = 0
    for k, (b, border, exp) in enumerate(golden_grid_batches()):
        res = check_obstacle_outcome(_env, outcome_params(), b, border, exp, "golden grid, call %d" % k)
        assert len(res) == (3 if border is not None else 4)
        total += b.n
    assert total == 7200


@pytest.mark.parametrize("geometry", GRID_MAPS, ids=lambda g: "%gm-%gm" % g)
def test_grid_windows(geometry):
    """Robot radii 0.6, 0.9 and 1.5 (the row loop after the unrolled eight), G = 90, 120 and 128, single cells at columns
    0, 63, 64, G - 1 and rows 0, G - 1 at and beside the window's edges, half-cell boundaries, corners, points outside
    the map, the border's equalities, and at G = 128 a robot of radius 9 whose window spans all 128 columns (the
    column mask must not shift by the width of its type)."""
    size, res = geometry
    params = outcome_params(map_size_m=size, map_resolution=res)
    for b, border, exp, notes, _ in grid_window_batches(size, res):
        tag = "windows %g / %g%s" % (size, res, ", border" if border else "")
        res_forms = check_obstacle_outcome(_env, params, b, border, exp, tag)
        ref = oracle_outcome(params, b, np.zeros((b.n, 2)), border)
        for form, o in res_forms.items():
            assert_outcome(o, ref, tag + " " + form)


@pytest.mark.parametrize("interleaved", [False, True], ids=["grouped", "interleaved"])
@pytest.mark.parametrize("N", ORDERED_COUNTS)
def test_ordered_reduction(N, interleaved):
    """Standing humans at exact binary gaps around a standing robot: dmin of every form bitwise equal to a plain walk of
    simulator/env.py:303-313 and to the oracle, info and done equal to the oracle's."""
    b, res = check_ordered(_env, N, interleaved, OUTCOME_FORMS)
    assert set(res) == set(OUTCOME_FORMS)


@pytest.mark.parametrize("time_limit", [25.0, 0.0], ids=["time_limit25", "time_limit0"])
@pytest.mark.parametrize("wall", ["grid", "border"])
@pytest.mark.parametrize("new_reward", [0, 1])
def test_reward_ladder(new_reward, wall, time_limit):
    """Colliding subset of {adult, bicycle, child, wall} x goal reached or not x which types stand inside their
    discomfort distance, then the exact thresholds, with four different penalties and three different factors; with
    time_limit = 0 every env reports INFO_TIMEOUT and a reward of 0 (the goal term under new_reward)."""
    params = ladder_params(new_reward, time_limit)
    b = ladder_batch(wall)
    ref, res = check_against_oracle(_env, params, b, np.zeros((b.n, 2)), LADDER_BORDER if wall == "border" else None,
                                    "ladder new_reward %d %s wall time_limit %g" % (new_reward, wall, time_limit))
    assert len(res) == (3 if wall == "border" else 4)
    if time_limit == 0:
        for o in res.values():
            assert (o["info"] == _abi.INFO_TIMEOUT).all() and o["done"].all()
            if not new_reward:
                assert (o["reward"] == 0).all()


@pytest.mark.parametrize("factor", [0.0, 0.5])
def test_unicycle_rotation_penalty(factor):
    """a1 == 0 and a1 != 0, rotation_penalty_factor zero and not, with and without a human inside its discomfort
    distance (danger wins)."""
    b, act = unicycle_batch()
    params = ladder_params(0, kinematics=_abi.UNICYCLE, rotation_penalty_factor=factor)
    ref, res = check_against_oracle(_env, params, b, act, None, "unicycle, factor %g" % factor)
    assert len(res) == 4 and ((ref["reward"] > 0).any() == (factor != 0))


def test_time_reward():
    """ROBOT_LINEAR robots that arrive at t = 0 ... 1.25 and never (time_good 0.5, time_max 1, time_limit 2), nine steps:
    per-step under either human policy and K = 9 as one launch, against the oracle and against each other."""
    ref = time_reward_forms(oracle_env, forms=("step",))["step"]
    res = time_reward_forms(_env)
    assert ref["info"].shape == (TIME_STEPS, len(ARRIVALS))
    for form, o in res.items():
        assert_outcome(o, ref, "time_reward " + form)
        for k in OUTCOME_KEYS:
            assert o[k].tobytes() == res["step"][k].tobytes(), (form, k)


def _guarded_case(which):
    if which == "ordered":
        b = ordered_batch(13, True)
        return outcome_params(), b, np.zeros((b.n, 2))
    b = ladder_batch("grid")
    return ladder_params(1), b, np.zeros((b.n, 2))


@pytest.mark.parametrize("which", ["ordered", "ladder"])
def test_device_outputs_stay_inside_their_buffers(which):
    """step_device (either human policy) and step_k_device (K = 2; per step and as one launch) with reward, done, info,
    dmin and dist_to_goal between canaries and poisoned inside: every element written, nothing beside the buffer, the
    host-output form's bytes."""
    import torch
    params, b, act = _guarded_case(which)
    E = b.n
    dt = dict(reward=torch.float64, done=torch.uint8, info=torch.uint8, dmin=torch.float64, dist_to_goal=torch.float64)
    shape = dict(reward=(E,), done=(E,), info=(E,), dmin=(E, 3), dist_to_goal=(E,))
    g = _env(params, E, b.N, b.S)
    g.use_torch_stream()
    for policy in (_abi.HUMAN_LINEAR, _abi.HUMAN_ORCA):
        g.reset(b)
        host = g.step(robot_action=act, human_policy=policy)
        g.reset(b)
        bufs = {k: Guarded(shape[k], dt[k]) for k in OUTCOME_KEYS}
        g.step_device({k: v.t for k, v in bufs.items()}, robot_action=torch.tensor(act, dtype=torch.float64, device="cuda"),
                      human_policy=policy)
        g.synchronize()
        for k, v in bufs.items():
            assert v.check().tobytes() == host[k].tobytes(), (which, "step_device", policy, k)
    K = 2
    acts = np.stack([act, act])
    for flags in (0, _abi.FLAG_ONE_LAUNCH):
        kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_EXTERNAL, flags=flags)
        g.reset(b)
        host = g.step_k(K, OUTCOME_KEYS, robot_action=acts, **kw)
        g.reset(b)
        bufs = {k: Guarded((K,) + shape[k], dt[k]) for k in OUTCOME_KEYS}
        g.step_k_device({k: v.t for k, v in bufs.items()}, K,
                        robot_action=torch.tensor(acts, dtype=torch.float64, device="cuda"), **kw)
        g.synchronize()
        for k, v in bufs.items():
            assert v.check().tobytes() == host[k].tobytes(), (which, "step_k_device", flags, k)
