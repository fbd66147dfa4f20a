"""The fused ORCA step writes the humans' next positions to a second pair of buffers, swapped by the host (-m gpu).

The STATE role of orca_step_kernel writes px_n / py_n and waits for the ROWS role only in the lanes whose env restarts;
the launcher swaps px / px_n and py / py_n behind the launch, and every other kernel and entry point goes on working on
px / py in place.  What can go wrong: a slot that is not carried over, a restart that writes the wrong buffer, or an
entry point that reads the buffer of the step before.  So
  - 40 fused steps of 25 envs (10 humans + 8 static rows, ragged), auto-reset with a time limit of 5 steps, with and
    without a custom pool: every output and the whole state against the oracle after every step;
  - after an odd and after an even number of fused steps, one call each of the linear-human step, the look-ahead (ORCA
    prelude, then cached), observe, ebc_step_k (per step and in one launch), the state read-back and a reset.
The bars are the project's for the oracle (tests/test_step_placement_gpu.py): masks exact, doubles within 1e-9 — the
ORCA velocities are floats, so a double that differs at all differs by 1e-8 and more: under HUMAN_ORCA with supplied
holonomic robot actions these are the oracle's bytes, and asserted as bytes — rotated rows within 1e-5 (the device's
atan2f / cosf / sinf are not glibc's); under HUMAN_LINEAR (cos / sin in double) the doubles are held to 1e-9."""
import numpy as np
import pytest

from ebcsim import _abi
from helpers import _close, load, oracle_env, params_of
from test_gpu_parity import _env, _synthetic_batch

pytestmark = pytest.mark.gpu

E, N, S = 25, 10, 8
AUTO = _abi.FLAG_AUTO_RESET


def _params():
    p = params_of(load("traj_n10_walls_t17_orcasub"))
    p.robot_kinematics = _abi.HOLONOMIC
    p.time_limit = 5 * p.time_step  # every env restarts every 5 steps at the latest
    return p


def _pair(pool, seed):
    params = _params()
    rs = np.random.RandomState(seed)
    b = _synthetic_batch(rs, E, N, S, n_lo=0, walls=True)
    g, o = _env(params, E, N, S), oracle_env(params, E, N, S)
    for env in (g, o):
        env.reset(b)
    if pool:
        scenes = _synthetic_batch(rs, 3 * E, N, S, n_lo=1, walls=True)
        for env in (g, o):
            env.set_scene_pool(scenes)
    return params, b, g, o


def same(got, ref, tag, exact=True):
    """Two dicts (or tuples) of outputs: bytes, rotated rows within 1e-5; exact=False: doubles within 1e-9."""
    if not isinstance(got, dict):
        got, ref = dict(enumerate(got)), dict(enumerate(ref))
    keys = [k for k in got if k in ref]
    assert keys, tag
    for k in keys:
        a, r = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == r.shape and a.dtype == r.dtype, (tag, k)
        if a.dtype == np.float32:
            np.testing.assert_allclose(a, r, atol=1e-5, rtol=1e-5, err_msg="%s %s" % (tag, k))
        elif exact or a.dtype != np.float64:
            bad = np.argwhere(a != r)
            assert a.tobytes() == r.tobytes(), "%s %s: %d values differ, the first at %s: %r, the oracle %r" % (
                tag, k, len(bad), bad[0].tolist() if len(bad) else "-0", a[tuple(bad[0])] if len(bad) else 0,
                r[tuple(bad[0])] if len(bad) else 0)
        else:
            np.testing.assert_allclose(a, r, atol=1e-9, rtol=0, err_msg="%s %s" % (tag, k))


def _acts(K, seed=5):
    return np.random.RandomState(seed).uniform(-0.7, 0.7, (K, E, 2))


def _fused(g, o, acts, tag, check=True, exact=True):
    for t, a in enumerate(acts):
        kw = dict(robot_action=a, human_policy=_abi.HUMAN_ORCA, flags=AUTO)
        out, ref = g.step(**kw), o.step(**kw)
        if check:
            same(out, ref, "%s fused step %d" % (tag, t), exact)
            same(g.get_state(), o.get_state(), "%s state after fused step %d" % (tag, t), exact)
    return ref


@pytest.mark.parametrize("pool", [False, True], ids=["own-scenes", "custom-pool"])
def test_forty_fused_steps_with_restarts(pool):
    _, _, g, o = _pair(pool, 4100 + pool)
    restarts, acts = 0, _acts(40)
    for t in range(40):
        restarts += int(_fused(g, o, acts[t:t + 1], "t%d" % t)["done"].sum())
    assert restarts >= 3 * E  # every env restarted several times, with both buffers as the target
    _close(g)


def _linear(g, o, a):
    kw = dict(robot_action=a, human_policy=_abi.HUMAN_LINEAR, flags=AUTO)
    same(g.step(**kw), o.step(**kw), "linear step", exact=False)
    same(g.get_state(), o.get_state(), "state after the linear step", exact=False)


def _lookahead(g, o, a):
    actions = np.random.RandomState(8).uniform(-0.7, 0.7, (9, 2))
    same(g.lookahead(actions, human_policy=_abi.HUMAN_ORCA), o.lookahead(actions, human_policy=_abi.HUMAN_ORCA),
         "look-ahead, ORCA prelude")
    same(g.lookahead(actions, human_policy=_abi.HUMAN_CACHED), o.lookahead(actions, human_policy=_abi.HUMAN_CACHED),
         "look-ahead, cached")
    kw = dict(robot_action=a, human_policy=_abi.HUMAN_CACHED, flags=AUTO)
    same(g.step(**kw), o.step(**kw), "cached step")
    same(g.get_state(), o.get_state(), "state after the cached step")


def _observe(g, o, a):
    same(g.observe(), o.observe(), "observe")


def _step_k(flags):
    def call(g, o, a):
        keys = ("reward", "done", "info", "state_rotated", "obs_rotated")
        kw = dict(robot_action=_acts(3, 9), human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_EXTERNAL)
        same(g.step_k(3, keys, flags=AUTO | flags, **kw), o.step_k(3, keys, flags=AUTO, **kw), "step_k flags %d" % flags)
        same(g.get_state(), o.get_state(), "state after step_k flags %d" % flags)
    return call


def _read_back(g, o, a):
    same(g.get_state(), o.get_state(), "state read-back")


def _reset(g, o, a):
    b = _synthetic_batch(np.random.RandomState(77), E, N, S, n_lo=0, walls=True)
    for env in (g, o):
        env.reset(b)
    same(g.get_state(), o.get_state(), "state after the reset")
    same(g.observe(), o.observe(), "observe after the reset")
    _fused(g, o, _acts(2, 10), "after the reset")


CALLS = [("linear", _linear), ("lookahead", _lookahead), ("observe", _observe), ("step_k", _step_k(0)),
         ("step_k_one_launch", _step_k(_abi.FLAG_ONE_LAUNCH)), ("read_back", _read_back), ("reset", _reset)]


@pytest.mark.parametrize("steps", [1, 2, 7], ids=["odd", "even", "odd-after-restarts"])
def test_every_entry_point_behind_fused_steps(steps):
    """One env pair per number of fused steps: before each call the pair is reset and stepped again."""
    params, b, g, o = _pair(True, 4200 + steps)
    acts = _acts(steps + 1, 6)
    for name, call in CALLS:
        for env in (g, o):
            env.reset(b)
        _fused(g, o, acts[:steps], name, check=False)
        call(g, o, acts[steps])
        # and the fused step goes on from what the call left
        _fused(g, o, _acts(2, 11), "behind " + name, exact=name != "linear")  # the linear humans' cos / sin: 1e-9
    _close(g)
