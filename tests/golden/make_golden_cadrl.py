#!/usr/bin/env python3
"""Generate the CADRL goldens (tests/golden/cadrl_*.npz) by importing the reference itself:

    python tests/golden/make_golden_cadrl.py --reference PATH_OF_THE_REFERENCE_TREE

The reference's own CADRL (rl/policy/cadrl.py) drives the reference's env with rvo2 substituted, like gen_sarl of
make_golden.py.  Neither tree ships a trained CADRL model: the network is the one its configure() builds after
torch.manual_seed(11).  No weight file is written.  A run's meta records the seed, the policy config text and, of the
reference's own get_model().state_dict(), every tensor's name, shape and SHA-256; tests/cadrl_cases.py builds the network
again from the seed and holds it to that record.

Three runs: the A5 and the N10 scene of the SARL goldens in phase "test" (several others: the minimum over the rows
decides), and the A5 config with ONE adult in phase "train" with epsilon 0, where `last_state` (cadrl.py:224-234, the
[13] vector of a two-agent state) exists; with several humans phase "train" ends in the reference's own assert, which
the generator checks.

A run is usable when its smallest top-2 gap exceeds twice the tolerance the tests hold the values to (8 x the error of
torch's float32 forward against a float64 copy of the same module, on the rows the reference's own network saw): the
generator asserts it and records both numbers.  Everything written is data."""
import argparse
import copy
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (A5, RVO2_MODE, SARL_RUNS, cfg_text, install_shims, jdump, save, scene_arrays,  # noqa: E402
                         write_tmp, info_code, parsed)
from ebcsim import config as ebc_config  # noqa: E402

POLICY_CONFIG = "configs/policy_configs/policy.config"
SEED = 11
TOL_FACTOR = 8
# (name, env config, overrides, test case, phase)
RUNS = [("cadrl_a5", SARL_RUNS[0][1], SARL_RUNS[0][2], SARL_RUNS[0][5], "test"),
        ("cadrl_n10", SARL_RUNS[1][1], SARL_RUNS[1][2], SARL_RUNS[1][5], "test"),
        ("cadrl_one", A5, {("sim", "adult_num"): 1}, 2, "train")]


def make(ref, text, phase):
    import torch
    from simulator.utils.test_utils import configure_env_policy_robot
    tmp = write_tmp(text)
    try:
        torch.manual_seed(SEED)
        env, pol, robot = configure_env_policy_robot(tmp, os.path.join(ref, POLICY_CONFIG), None, phase=phase, policy="cadrl")
    finally:
        os.unlink(tmp)
    pol.set_epsilon(0.0)
    return env, pol, robot


def gen_cadrl(ref):
    import torch
    RVO2_MODE["substitute"] = True
    pol_text = cfg_text(os.path.join(ref, POLICY_CONFIG))
    for name, env_path, overrides, case, phase in RUNS:
        text = cfg_text(os.path.join(ref, env_path), overrides)
        env, pol, robot = make(ref, text, phase)
        m64 = copy.deepcopy(pol.get_model()).double()
        err = {"rows": 0.0, "min": 0.0, "calls": 0}

        def watch(module, inputs, output):
            with torch.no_grad():
                o64 = m64(inputs[0].double())
            err["rows"] = max(err["rows"], float((output.detach().double() - o64).abs().max()))
            err["min"] = max(err["min"], float((output.detach().double().min() - o64.min()).abs()))
            err["calls"] += 1
        pol.get_model().register_forward_hook(watch)
        ob, _ = env.reset("test", test_case=case, compute_local_map=False)
        init = scene_arrays(env)
        acts, vals, infos, rewards, last = [], [], [], [], []
        done = False
        while not done and len(acts) < 200:
            action = robot.act(ob, env=env)
            acts.append([action[0], action[1]])
            vals.append(list(pol.action_values))
            if phase == "train":
                last.append(pol.last_state.numpy().astype(np.float32))
            ob, _, reward, done, info = env.step(action, compute_local_map=False)
            infos.append(info_code(info))
            rewards.append(reward)
        v = np.sort(np.array(vals), axis=1)
        gap = float(np.min(v[:, -1] - v[:, -2]))
        tol = TOL_FACTOR * err["rows"]
        print("  %s: %d rows per state, %d decisions, final info code %d, smallest top-2 gap %.3g, float32 error per row %.3g "
              "(of the minimum %.3g), tolerance %.3g" % (name, len(ob), len(acts), infos[-1], gap, err["rows"], err["min"], tol))
        assert err["calls"] == 81 * len(acts)
        assert gap > 2 * tol, "%s: pick another test case (gap %.3g <= 2 x tolerance %.3g)" % (name, gap, tol)
        params = ebc_config.params_from_config(parsed(text), parsed(pol_text), policy="cadrl")
        out = {("init_" + k): v for k, v in init.items()}
        out.update(action=np.array(acts), values=np.array(vals), info=np.array(infos), reward=np.array(rewards, float),
                   action_space=np.array([[a[0], a[1]] for a in pol.action_space]),
                   params=jdump(ebc_config.params_to_dict(params)),
                   meta=jdump({"config": env_path, "config_text": text, "policy_config": POLICY_CONFIG,
                               "policy_config_text": pol_text, "gamma": pol.gamma, "phase": phase,
                               "seed_case": case, "torch_seed": SEED, "rows": len(ob),
                               "state_dict": [[k, list(t.shape), hashlib.sha256(t.detach().numpy().tobytes()).hexdigest()]
                                              for k, t in pol.get_model().state_dict().items()],
                               "final_info": infos[-1], "top2_gap": gap, "float32_error": err["rows"]}))
        if phase == "train":
            out["last_state"] = np.stack(last)
        save(name, **out)
        if phase == "test":  # the same scene in phase "train": transform() asserts one other agent (cadrl.py:231)
            env, pol, robot = make(ref, text, "train")
            ob, _ = env.reset("test", test_case=case, compute_local_map=False)
            try:
                robot.act(ob, env=env)
            except AssertionError:
                print("  %s in phase train: the reference's AssertionError, as expected" % name)
            else:
                raise SystemExit("%s in phase train did not assert" % name)
    RVO2_MODE["substitute"] = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    args.reference = os.path.abspath(args.reference)
    install_shims()
    sys.path.insert(0, args.reference)
    os.chdir(args.reference)  # the reference resolves config paths relative to its root
    import logging
    logging.disable(logging.CRITICAL)
    gen_cadrl(args.reference)


if __name__ == "__main__":
    main()
