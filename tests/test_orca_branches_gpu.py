"""orca_group<GS> (csrc/ebc_orca_group.h) at every instantiated group size and in every branch of RVO2 (-m gpu).

The four kernels that call it — orca_step_kernel (the step), orca_kernel (the look-ahead prelude), rollout_kernel
(EBC_FLAG_ONE_LAUNCH) and orca_robot_kernel (the demonstrator) — are held to the plain oracle BIT FOR BIT
(assert_array_equal; ORCA has no transcendental) on the batches of tests/helpers.py: dense crowds, exact lattices,
coincident humans, ragged counts, a partly filled last wave.  The human counts reach all 13 group sizes, each both full
and with spare lanes; tests/test_orca_branches_cpu.py asserts, from the traced oracle alone, that these very batches reach
linearProgram3, every way linearProgram1 fails, colliding and parallel lines, maxNeighbors truncation, exact distance ties
and NaN lines.  A difference here is a finding about orca_group, not about the oracle: where a line is NaN (two agents
with one position and one velocity) the oracle's fminf / fmaxf is RVO2's std::min / std::max.

Parameter sets (helpers.ORCA_PARAM_SETS): maxNeighbors / neighborDist, and time_step, orca_time_horizon and
orca_safety_space off their defaults one at a time and together; the robot kernel also under a handle whose safety space
is not the robot's own.

Tie order: both sides rank equal distances in insertion order.  RVO2 proper walks a kd-tree once it holds more than 10
agents (N >= 11 here), and visits ties in the tree's order; that order is knowingly not modelled, so the lattice cases
hold the two sides to each other, not to RVO2."""
import numpy as np
import pytest

from ebcsim import _abi, actions as ebc_actions
from helpers import (ORCA_GROUP_SIZES, ORCA_HUMAN_CASES, ORCA_ROBOT_CASES, ORCA_ROBOT_MOVED_CASES, ORCA_STEPS, Guarded,
                     orca_case_id, orca_case_params, orca_group_size, orca_human_batch, orca_reference,
                     orca_robot_actions, orca_robot_batch, orca_robot_case_id, orca_robot_reference)
from test_gpu_parity import _compare_step, _env

pytestmark = pytest.mark.gpu

ONE = _abi.FLAG_ONE_LAUNCH
human_cases = pytest.mark.parametrize("case", ORCA_HUMAN_CASES, ids=orca_case_id)


def _bitwise(got, want, tag):
    """assert_array_equal (NaN positions equal), with the first differing (env, human) in the message."""
    got, want = np.asarray(got), np.asarray(want)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    msg = tag
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        msg = "%s: %d of %d differ, first at %s: %r != %r, max |diff| %g" % (
            tag, int(bad.sum()), bad.size, at, got[at], want[at], float(np.nanmax(np.abs(np.where(bad, got - want, 0)))))
    np.testing.assert_array_equal(got, want, err_msg=msg)


def _setup(case):
    N, rv, ps = case
    b = orca_human_batch(N, rv)
    g = _env(orca_case_params(rv, ps), b.n, N, 0)
    g.reset(b)
    return g, b, orca_robot_actions(b.n), orca_reference(case)


def _state_bars(g, want, tag):
    got = g.get_state()
    for k in got:
        np.testing.assert_allclose(got[k], want[k], atol=1e-9, rtol=0, err_msg=tag + " state " + k)


@human_cases
def test_step_kernel(case):
    """step(HUMAN_ORCA, supplied robot action) from reset, three times: human_action bitwise, every other output and the
    state at the bars of test_gpu_parity._compare_step."""
    g, b, act, ref = _setup(case)
    for t in range(ORCA_STEPS):
        tag = "%s step %d" % (orca_case_id(case), t)
        out = g.step(robot_action=act[t], human_policy=_abi.HUMAN_ORCA)
        _bitwise(out["human_action"], ref["out"][t]["human_action"], tag + " human_action")
        _compare_step(out, ref["out"][t], tag)
        _state_bars(g, ref["state"][t], tag)


@human_cases
def test_lookahead_prelude(case):
    """lookahead(HUMAN_ORCA) leaves every human's ORCA velocity in the cache; step(HUMAN_CACHED) then reports it."""
    g, b, act, ref = _setup(case)
    g.lookahead(ebc_actions.build_action_space(0.7), human_policy=_abi.HUMAN_ORCA, want_rows=False)
    out = g.step(robot_action=act[0], human_policy=_abi.HUMAN_CACHED)
    _bitwise(out["human_action"], ref["out"][0]["human_action"], orca_case_id(case) + " cached human_action")


@human_cases
def test_one_launch(case):
    """step_k(K = 2) as one launch: the humans' velocities and positions are the oracle's after two steps, bit for bit,
    and the per-step form's, byte for byte."""
    g, b, act, ref = _setup(case)
    per_step = _env(g.params, b.n, b.N, 0)
    per_step.reset(b)
    kw = dict(robot_action=act[:2], human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_EXTERNAL)
    g.step_k(2, ("reward",), flags=ONE, **kw)
    per_step.step_k(2, ("reward",), flags=0, **kw)
    got, other, want = g.get_state(), per_step.get_state(), ref["state"][1]
    for k in ("vx", "vy", "px", "py"):
        _bitwise(got[k], want[k], "%s one launch %s" % (orca_case_id(case), k))
        assert got[k].tobytes() == other[k].tobytes(), "%s: one launch and per-step %s differ" % (orca_case_id(case), k)


@pytest.mark.parametrize("safety", [0.0, 0.15])
@pytest.mark.parametrize("case", ORCA_ROBOT_CASES + ORCA_ROBOT_MOVED_CASES, ids=orca_robot_case_id)
def test_robot_kernel(case, safety):
    """robot_orca(safety) with the robot inside the crowd; rows N + S = 1 .. 13, 16, 17, 21, 22, 32.  The cases with a
    parameter set run under a handle whose own safety space (the humans': 0.1) is not the robot's, with the time step and
    the horizon moved too under "all": the robot's solve takes `safety` and the handle's step and horizon."""
    N, S = case[:2]
    b = orca_robot_batch(N, S)
    g = _env(orca_case_params(0, *case[2:]), b.n, N, S)
    g.reset(b)
    _bitwise(g.robot_orca(safety), orca_robot_reference(case, safety),
             "robot %s safety %g" % (orca_robot_case_id(case), safety))


@pytest.mark.parametrize("N", [4, 10])
def test_forced_group_size(N, monkeypatch):
    """EBCSIM_ORCA_GROUP (read at ebc_create) runs the same humans in every instantiated group size from the natural one
    up: the step's and the prelude's human_action are the oracle's at each, hence byte-identical across sizes."""
    case = (N, 0, "default")
    b, act, ref = orca_human_batch(N, 0), orca_robot_actions(orca_human_batch(N, 0).n), orca_reference(case)
    sizes = [gs for gs in ORCA_GROUP_SIZES if gs >= orca_group_size(N - 1)]
    assert len(sizes) == {4: 12, 10: 6}[N]
    seen = set()
    for gs in sizes:
        monkeypatch.setenv("EBCSIM_ORCA_GROUP", str(gs))
        for prelude in (False, True):
            g = _env(orca_case_params(), b.n, N, 0)
            g.reset(b)
            if prelude:
                g.lookahead(ebc_actions.build_action_space(0.7), human_policy=_abi.HUMAN_ORCA, want_rows=False)
            out = g.step(robot_action=act[0], human_policy=_abi.HUMAN_CACHED if prelude else _abi.HUMAN_ORCA)
            _bitwise(out["human_action"], ref["out"][0]["human_action"],
                     "N %d in %d-lane groups%s" % (N, gs, ", prelude" if prelude else ""))
            seen.add(out["human_action"].tobytes())
    assert len(seen) == 1


@pytest.mark.parametrize("gs", ORCA_GROUP_SIZES)
def test_device_output_stays_inside_its_buffer(gs):
    """The device-output form of the step, one full group per size (N - 1 = GS others): human_action between canaries and
    poisoned inside — all of it written, nothing beside it, the oracle's bits."""
    import torch
    case = (gs + 1, 0, "default")
    g, b, act, ref = _setup(case)
    g.use_torch_stream()
    buf = Guarded((b.n, b.N, 2), torch.float64, tile_rows=1)
    g.step_device({"human_action": buf.t}, robot_action=torch.tensor(act[0], dtype=torch.float64, device="cuda"),
                  human_policy=_abi.HUMAN_ORCA)
    g.synchronize()
    _bitwise(buf.check(), ref["out"][0]["human_action"], "%d-lane groups, device human_action" % gs)
