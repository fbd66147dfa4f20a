"""Humans on a policy per entity type (EBC_HUMAN_BY_TYPE) without a GPU: the checker's composition (tests/mixed_humans.py)
and the facade on top of it against the reference's own run of a mixed scene (tests/golden/traj_mixed_a3b3c2.npz, made by
tests/golden/make_golden_mixed.py), the config helper, and the new code and entry in header and bindings.  Bars as in
tests/test_oracle_golden.py and tests/test_facade.py: masks and codes exact, float64 values 1e-12 (the facade's 1e-9),
float32 rotated rows 1e-5."""
import configparser
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from ebcsim import _abi, _capi, config as ebc_config
from ebcsim import env as ebc_env
from ebcsim.action import ActionXY
from ebcsim.agents import Robot
from ebcsim.policy import policy_factory
from helpers import batch_from_init, check_trajectory, load, params_of
from mixed_humans import BY_TYPE, LINEAR, ORCA, AsMixed, MixedOracle, config_text_of_mixed, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "traj_mixed_a3b3c2"


def test_fixture_is_a_mixed_scene():
    z = load(NAME)
    meta = json.loads(str(z["meta"]))
    assert table_of(z) == (ORCA, LINEAR, ORCA) and meta["human_policy"] == "by_type"
    assert list(z["init_type"]) == [0, 0, 0, 1, 1, 1, 2, 2] and len(z["action"]) == 40
    assert meta["overrides"]["bicycles.policy"] == "linear" and meta["overrides"]["adults.policy"] == "orca"
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", NAME + ".npz")) < 100 * 1024


def test_checker_composition_reproduces_the_reference():
    """Reference orchestration of a mixed scene end to end (rvo2 replaced by the oracle's restatement, as for the
    `_orcasub` fixtures): who is whose neighbour with which velocity, and the order of the updates."""
    z = load(NAME)
    b = batch_from_init(z)
    env = MixedOracle(params_of(z), 1, b.N, b.S)
    env.reset(b)
    check_trajectory(AsMixed(env, table_of(z)), z, atol=1e-12)


def test_uniform_tables_are_the_plain_policies_in_the_checker():
    z = load(NAME)
    b = batch_from_init(z)
    for code in (ORCA, LINEAR):
        mixed, plain = MixedOracle(params_of(z), 1, b.N, b.S), MixedOracle(params_of(z), 1, b.N, b.S)
        mixed.set_human_policies(code, code, code)
        for env in (mixed, plain):
            env.reset(b)
        for t in range(6):
            om = mixed.step(robot_action=z["action"][t][None], human_policy=BY_TYPE)
            op = plain.step(robot_action=z["action"][t][None], human_policy=code)
            assert all(om[k].tobytes() == op[k].tobytes() for k in op), t


def _facade(text, backend):
    cfg = configparser.RawConfigParser()
    cfg.read_string(text)
    env = ebc_env.make(backend_factory=backend)
    env.configure(cfg)
    robot = Robot(cfg, "robot")
    env.set_robot(robot)
    pol = policy_factory["linear"]()
    robot.set_policy(pol)
    pol.set_phase("test")
    return env, robot


def test_facade_reproduces_the_reference_through_the_checker():
    z = load(NAME)
    meta = json.loads(str(z["meta"]))
    made = []

    def backend(params, E, N, S):
        made.append(MixedOracle(params, E, N, S))
        return made[-1]
    env, robot = _facade(config_text_of_mixed(z), backend)
    ob, _ = env.reset("test", test_case=meta["seed_case"])
    assert made[0].human_policies == table_of(z)  # the facade applied the config's table
    n = len(z["init_px"])
    np.testing.assert_array_equal([o.px for o in ob[:n]], z["init_px"])
    assert [h.policy.name for h in env.scene.adults + env.scene.bicycles + env.scene.children] == ["ORCA"] * 3 + ["LINEAR"] * 3 + ["ORCA"] * 2
    la_steps = list(z["la_step"])
    evaluations = 0
    for t in range(len(z["action"])):
        if t in la_steps:
            k = la_steps.index(t)
            for ai in (0, 7, 40, 80):
                nob, r, d, inf = env.onestep_lookahead(ActionXY(*z["la_actions"][ai]))
                assert d == bool(z["la_done"][k][ai])
                np.testing.assert_allclose(r, z["la_reward"][k][ai], atol=1e-9)
                np.testing.assert_allclose([[o.px, o.py, o.vx, o.vy, o.radius] for o in nob], z["la_next_ob"][k][:, :5], atol=1e-9)
        ob, local_map, reward, done, info = env.step(ActionXY(*z["action"][t]))
        evaluations += 1  # once per state: the four look-aheads and the step share the first evaluation
        assert env.orca_evaluations == evaluations
        assert done == bool(z["done"][t]) and int(z["info"][t]) == 0 and type(info).__name__ == "Nothing"
        np.testing.assert_allclose(reward, z["reward"][t], atol=1e-9)
        rows = np.array([[o.px, o.py, o.vx, o.vy, o.radius, int(o.obj_type)] for o in ob])
        np.testing.assert_allclose(rows, z["ob"][t], atol=1e-9)
        np.testing.assert_allclose(env.global_time, z["time"][t], atol=1e-12)
        np.testing.assert_allclose([robot.px, robot.py, robot.vx, robot.vy, robot.theta], z["robot"][t][[0, 1, 2, 3, 8]], atol=1e-9)


def test_facade_keeps_refusing_a_mix_on_a_backend_without_the_table():
    from oracle import oracle
    z = load(NAME)
    env, _ = _facade(config_text_of_mixed(z), lambda params, E, N, S: oracle.OracleEnv(params, E, N, S))
    with pytest.raises(NotImplementedError, match="linear.*orca"):
        env.reset("test", test_case=1)


def _cfg(**policies):
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "mixed_a3b3c2.config"))
    for key, val in policies.items():
        sec, opt = key.split("__")
        cfg.set(sec, opt, str(val))
    return cfg


def test_config_helper():
    f = ebc_config.human_policies_from_config
    assert f(_cfg()) == (BY_TYPE, (ORCA, LINEAR, ORCA))  # the shipped mixed config
    assert f(_cfg(bicycles__policy="orca")) == (ORCA, (ORCA, ORCA, ORCA))
    assert f(_cfg(adults__policy="linear", children__policy="linear")) == (LINEAR, (LINEAR, LINEAR, LINEAR))
    assert f(_cfg(adults__policy="linear")) == (BY_TYPE, (LINEAR, LINEAR, ORCA))
    # a type the scene does not have is not read (env.py:88-92): uniform again, and its name may be anything
    assert f(_cfg(sim__bicycle_num=0)) == (ORCA, (ORCA, ORCA, ORCA))
    assert f(_cfg(sim__bicycle_num=0, bicycles__policy="none")) == (ORCA, (ORCA, ORCA, ORCA))
    assert f(_cfg(sim__adult_num=0, sim__children_num=0)) == (LINEAR, (LINEAR, LINEAR, LINEAR))
    assert f(_cfg(sim__children_num=0, adults__policy="linear", bicycles__policy="orca")) == (BY_TYPE, (LINEAR, ORCA, ORCA))
    assert f(_cfg(sim__adult_num=0, sim__bicycle_num=0, sim__children_num=0)) == (ORCA, (ORCA, ORCA, ORCA))
    for name in ("none", "orca_obstacles", "socialforce"):
        with pytest.raises(NotImplementedError, match=name):
            f(_cfg(children__policy=name))
    # every shipped env config is uniform ORCA and keeps the plain code
    for name in ("bench_metric", "bench_cfg2", "sarl_a5", "sarl_h24", "cadrl_one_human"):
        cfg = configparser.RawConfigParser()
        cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", name + ".config"))
        assert f(cfg)[0] in (ORCA, LINEAR) and len(set(f(cfg)[1])) == 1, name


def test_header_bindings_and_library_agree():
    with open(os.path.join(ROOT, "include", "ebcsim.h")) as fh:
        header = fh.read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"EBC_HUMAN_(\w+) = (\d+)", header)}
    assert codes == {"EXTERNAL": _abi.HUMAN_EXTERNAL, "LINEAR": _abi.HUMAN_LINEAR, "ORCA": _abi.HUMAN_ORCA,
                     "CACHED": _abi.HUMAN_CACHED, "BY_TYPE": _abi.HUMAN_BY_TYPE}
    assert _abi.HUMAN_BY_TYPE == 4 and "#define EBC_ABI_VERSION 1" in header
    assert re.search(r"int ebc_set_human_policies\(void \*handle, const int32_t policy_of_type\[3\]\);", header)
    lib = _capi.lib()
    assert lib.ebc_abi_version() == 1
    table = (C.c_int32 * 3)(ORCA, LINEAR, ORCA)
    assert lib.ebc_set_human_policies(None, table) == _abi.ERR_INVALID and b"null handle" in lib.ebc_last_error()
