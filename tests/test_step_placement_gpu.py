"""The fused ORCA step at the shapes where the spans of its grid (csrc/ebc_step_grid.h: eight classes of
ceil(E / 8) envs, every role dealt to them by block index mod 8) can go wrong, every output every step against the
oracle as test_gpu_parity.test_orca_step_roles_without_rows_and_wide_envs holds it: `done` exact, reward / ob /
human_action / the final state at 1e-9, obs_rotated at 1e-5; a synchronize() after every step reports a mailbox
time-out.  12 steps with auto-reset (episodes of 5 steps, so every env restarts) and ragged human counts, steps
with and without the row outputs alternating."""
import numpy as np
import pytest

from ebcsim import _abi
from helpers import load, params_of
from test_gpu_parity import _env, _synthetic_batch

pytestmark = pytest.mark.gpu

STEPS = 12

CASES = [
    # E, N, S, n_lo, walls, custom pool
    pytest.param(1, 10, 8, 3, True, False, id="E1-seven-empty-classes"),
    pytest.param(7, 7, 3, 0, True, False, id="E7-fewer-envs-than-classes"),
    pytest.param(9, 10, 8, 0, True, False, id="E9-ec2-class4-partial-5to7-empty"),
    # ec = 17 is a multiple of none of 16 (ENV), 3 (ROWS), 6 (STATE) envs per wave, and 170 humans of none of 7:
    # a partial wave of every role at every class end, ORCA groups clipped mid-wave
    pytest.param(129, 10, 8, 0, True, False, id="E129-partial-wave-at-every-class-end"),
    pytest.param(64, 5, 0, 0, True, False, id="E64-N5-no-static"),
    pytest.param(6, 33, 95, 28, False, False, id="E6-N33-S95-one-env-per-rows-wave"),
    # ec = 3: envs walk a pool of 3 E scenes with stride E, cursors and restart scenes of every class side by side
    pytest.param(20, 8, 4, 1, True, True, id="E20-custom-pool-across-class-ends"),
]


@pytest.mark.parametrize("E,N,S,n_lo,walls,pool", CASES)
def test_step_spans_vs_oracle(E, N, S, n_lo, walls, pool):
    from oracle import oracle
    params = params_of(load("traj_n10_walls_t17_orcasub"))
    params.time_limit = 5 * params.time_step  # every env ends an episode at least twice in 12 steps
    rs = np.random.RandomState(1000 * E + N)
    b = _synthetic_batch(rs, E, N, S, n_lo=n_lo, walls=walls)
    g = _env(params, E, N, S)
    o = oracle.OracleEnv(params, E, N, S)
    for env in (g, o):
        env.reset(b)
    if pool:
        scenes = _synthetic_batch(rs, 3 * E, N, S, n_lo=1, walls=walls)
        for env in (g, o):
            env.set_scene_pool(scenes)
    g.use_torch_stream()
    slim = g.alloc_step_outputs(("reward", "done"))
    full = g.alloc_step_outputs(("reward", "done", "info", "ob", "obs_rotated", "human_action"))
    fl = _abi.FLAG_AUTO_RESET
    restarts = 0
    for t in range(STEPS):
        outs = full if t % 2 else slim
        g.step_device(outs, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=fl)
        ref = o.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=fl)
        g.synchronize()  # also reports a mailbox timeout
        tag = "step %d" % t
        np.testing.assert_array_equal(outs["done"].cpu().numpy(), ref["done"], err_msg=tag)
        np.testing.assert_allclose(outs["reward"].cpu().numpy(), ref["reward"], atol=1e-9, rtol=0, err_msg=tag)
        if outs is full:
            np.testing.assert_array_equal(outs["info"].cpu().numpy(), ref["info"], err_msg=tag)
            np.testing.assert_allclose(outs["ob"].cpu().numpy(), ref["ob"], atol=1e-9, rtol=0, err_msg=tag)
            np.testing.assert_allclose(outs["human_action"].cpu().numpy(), ref["human_action"], atol=1e-9, rtol=0, err_msg=tag)
            np.testing.assert_allclose(outs["obs_rotated"].cpu().numpy(), ref["obs_rotated"], atol=1e-5, rtol=1e-5, err_msg=tag)
        restarts += int(ref["done"].sum())
    assert restarts >= 2 * E  # the restart path ran in every env
    sg, so = g.get_state(), o.get_state()
    for k in sg:
        np.testing.assert_allclose(sg[k], so[k], atol=1e-9, rtol=0, err_msg=k)
