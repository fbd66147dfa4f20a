#!/usr/bin/env python3
"""Generate the SAIL goldens (tests/golden/sail_a5.npz, sail_cases.npz) by importing the reference itself:

    python tests/golden/make_golden_sail.py --reference PATH_OF_THE_REFERENCE_TREE

The reference's own SAIL (rl/policy/sail.py) drives the reference's env with rvo2 substituted, like gen_sarl of
make_golden.py.  Neither tree ships a trained SAIL model: the network is the one its configure() builds after
torch.manual_seed(11) from configs/policy_configs/policy_sail.config ([sail] adult_num = 5).  Its state_dict is recorded
as arrays (38 k float32: model weights are data), under "sd/<key>".

sail_a5: the A5 scene of the SARL goldens (its 5 rows equal adult_num), at most 200 steps.  Per step: last_state[0] [6]
and last_state[1] [5, 4] (float32, SAIL.transform), the action, feat_joint [64] (a forward hook on the model), the float64
robot state [9] and observation [5, 5] the decision was made from, reward and info.

sail_cases: constructed states at adult_num = 5 through the reference's own predict(): an arrived robot on either side of
the radius (not on it), coincident agents, zero velocities, large coordinates.  `decided` is 0 where predict() returned
the arrival action before the network ran (feat_joint is NaN there).

The generator also asserts that the 18-row N10 scene makes the reference raise.  Everything written is data."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (RVO2_MODE, SARL_RUNS, cfg_text, install_shims, jdump, save, scene_arrays,  # noqa: E402
                         write_tmp, info_code, parsed)
from ebcsim import config as ebc_config  # noqa: E402

POLICY_CONFIG = "configs/policy_configs/policy_sail.config"
SEED = 11


def make(ref, text):
    import torch
    from simulator.utils.test_utils import configure_env_policy_robot
    tmp = write_tmp(text)
    try:
        torch.manual_seed(SEED)
        env, pol, robot = configure_env_policy_robot(tmp, os.path.join(ref, POLICY_CONFIG), None, phase="test", policy="sail")
    finally:
        os.unlink(tmp)
    return env, pol, robot


def hooked(pol):
    """Every forward of the policy's model -> seen: (robot_state [6], crowd [N, 4], action [2], feat_joint [64])."""
    seen = []

    def watch(module, inputs, output):
        seen.append((inputs[0].detach().numpy().copy(), inputs[1].detach().numpy().copy(),
                     output[0].detach().numpy().reshape(2).copy(), output[1].detach().numpy().reshape(-1).copy()))
    pol.get_model().register_forward_hook(watch)
    return seen


def robot_array(r):
    return np.array([r.px, r.py, r.vx, r.vy, r.radius, r.gx, r.gy, r.v_pref, r.theta], dtype=np.float64)


def ob_array(ob):
    return np.array([[o.px, o.py, o.vx, o.vy, o.radius] for o in ob], dtype=np.float64)


def gen_run(ref, pol_text):
    name, env_path, overrides, case = "sail_a5", SARL_RUNS[0][1], SARL_RUNS[0][2], SARL_RUNS[0][5]
    text = cfg_text(os.path.join(ref, env_path), overrides)
    env, pol, robot = make(ref, text)
    seen = hooked(pol)
    ob, _ = env.reset("test", test_case=case, compute_local_map=False)
    init = scene_arrays(env)
    rec = {k: [] for k in ("last_robot", "last_agents", "action", "feat_joint", "robot", "ob", "reward", "info")}
    done = False
    while not done and len(rec["action"]) < 200:
        rec["robot"].append(robot_array(robot))
        rec["ob"].append(ob_array(ob))
        action = robot.act(ob, env=env)
        assert len(seen) == len(rec["action"]) + 1, "a step decided without the network (arrival): pick another case"
        rec["last_robot"].append(pol.last_state[0].numpy().copy())
        rec["last_agents"].append(pol.last_state[1].numpy().copy())
        rec["action"].append([action[0], action[1]])
        rec["feat_joint"].append(seen[-1][3])
        assert np.array_equal(np.float32(rec["action"][-1]), seen[-1][2])
        ob, _, reward, done, info = env.step(action, compute_local_map=False)
        rec["info"].append(info_code(info))
        rec["reward"].append(reward)
    sd = {k: v.detach().numpy().copy() for k, v in pol.get_model().state_dict().items()}
    print("  %s: %d rows per state, %d decisions, final info code %d, %d weights" % (
        name, len(rec["ob"][0]), len(rec["action"]), rec["info"][-1], sum(v.size for v in sd.values())))
    params = ebc_config.params_from_config(parsed(text), parsed(pol_text), policy="sail")
    out = {("init_" + k): v for k, v in init.items()}
    out.update({("sd/" + k): v for k, v in sd.items()})
    out.update(last_robot=np.stack(rec["last_robot"]).astype(np.float32), last_agents=np.stack(rec["last_agents"]).astype(np.float32),
               action=np.array(rec["action"], dtype=np.float64), feat_joint=np.stack(rec["feat_joint"]).astype(np.float32),
               robot=np.stack(rec["robot"]), ob=np.stack(rec["ob"]), reward=np.array(rec["reward"], float), info=np.array(rec["info"]),
               params=jdump(ebc_config.params_to_dict(params)),
               meta=jdump({"config": env_path, "config_text": text, "policy_config": POLICY_CONFIG, "policy_config_text": pol_text,
                           "seed_case": case, "torch_seed": SEED, "rows": len(rec["ob"][0]), "adult_num": 5,
                           "state_dict": list(sd), "final_info": rec["info"][-1], "kinematics": pol.kinematics}))
    save(name, **out)
    return pol, sd


def gen_cases(pol, sd):
    """Constructed joint states through the same policy object's predict()."""
    from simulator.utils.state import FullState, JointState, ObservableState
    seen = hooked(pol)
    rs = np.random.RandomState(5)
    names, robots, obs = [], [], []

    def add(name, robot, ob):
        names.append(name)
        robots.append(np.array(robot, dtype=np.float64))
        obs.append(np.array(ob, dtype=np.float64))

    def crowd():
        o = rs.uniform(-4.0, 4.0, (5, 5))
        o[:, 2:4] = rs.uniform(-1.0, 1.0, (5, 2))
        o[:, 4] = 0.3
        return o
    base = [0.5, -3.0, 0.2, 0.9, 0.3, 0.0, 4.0, 1.0, 1.2]
    add("plain", base, crowd())
    # on either side of the radius, not on it: |robot - goal| = 0.29 and 0.31 against radius 0.3
    add("arrived_inside", [0.0, 4.0 - 0.29, 0.1, 0.4, 0.3, 0.0, 4.0, 1.0, 1.5], crowd())
    add("arrived_outside", [0.0, 4.0 - 0.31, 0.1, 0.4, 0.3, 0.0, 4.0, 1.0, 1.5], crowd())
    add("arrived_diagonal_inside", [1.0 + 0.2, 2.0 - 0.2, 0.0, 0.0, 0.3, 1.0, 2.0, 1.0, 0.0], crowd())
    o = crowd()
    o[3] = o[1]
    add("coincident_two", base, o)
    o = crowd()
    o[:] = o[2]
    add("coincident_all", base, o)
    o = crowd()
    o[0, :2] = base[:2]
    add("agent_on_robot", base, o)
    o = crowd()
    o[:, 2:4] = 0.0
    add("zero_velocities", [0.5, -3.0, 0.0, 0.0, 0.3, 0.0, 4.0, 1.0, 0.0], o)
    o = crowd()
    o[:, :2] += 1.0e4
    add("large_coordinates", [1.0e4 + 0.5, 1.0e4 - 3.0, 0.2, 0.9, 0.3, 1.0e4, 1.0e4 + 4.0, 1.0, 1.2], o)
    o = crowd()
    o[:, :2] *= 1.0e3
    add("far_agents", base, o)
    for q in range(6):
        add("random_%d" % q, [rs.uniform(-5, 5), rs.uniform(-5, 5), rs.uniform(-1, 1), rs.uniform(-1, 1), 0.3,
                              rs.uniform(-5, 5), rs.uniform(-5, 5), 1.0, rs.uniform(-3, 3)], crowd())
    actions, feats, decided = [], [], []
    for name, r, o in zip(names, robots, obs):
        state = JointState(FullState(*[float(x) for x in r]), [ObservableState(*[float(x) for x in row]) for row in o])
        n = len(seen)
        action = pol.predict(state)
        ran = len(seen) == n + 1
        assert ran != name.startswith("arrived_") or name == "arrived_outside", name
        actions.append([action[0], action[1]])
        decided.append(int(ran))
        feats.append(seen[-1][3] if ran else np.full(64, np.nan, dtype=np.float32))
    print("  sail_cases: %d states, %d decided by the network" % (len(names), sum(decided)))
    out = {("sd/" + k): v for k, v in sd.items()}
    out.update(robot=np.stack(robots), ob=np.stack(obs), action=np.array(actions, dtype=np.float64),
               feat_joint=np.stack(feats).astype(np.float32), decided=np.array(decided, dtype=np.uint8),
               meta=jdump({"names": names, "torch_seed": SEED, "adult_num": 5, "policy_config": POLICY_CONFIG, "state_dict": list(sd)}))
    save("sail_cases", **out)


def check_n10_raises(ref):
    """The 18-row N10 scene: the reference's network is built for exactly 5 rows and raises."""
    _, env_path, overrides, _, _, case, _ = SARL_RUNS[1]
    env, pol, robot = make(ref, cfg_text(os.path.join(ref, env_path), overrides))
    ob, _ = env.reset("test", test_case=case, compute_local_map=False)
    assert len(ob) == 18, len(ob)
    try:
        robot.act(ob, env=env)
    except RuntimeError as e:
        print("  the N10 scene (%d rows): the reference raises %s, as expected" % (len(ob), type(e).__name__))
    else:
        raise SystemExit("the N10 scene did not make the reference raise")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    install_shims()
    sys.path.insert(0, ref)
    os.chdir(ref)  # the reference resolves config paths relative to its root
    import logging
    logging.disable(logging.CRITICAL)
    RVO2_MODE["substitute"] = True
    pol_text = cfg_text(os.path.join(ref, POLICY_CONFIG))
    pol, sd = gen_run(ref, pol_text)
    gen_cases(pol, sd)
    check_n10_raises(ref)
    RVO2_MODE["substitute"] = False


if __name__ == "__main__":
    main()
