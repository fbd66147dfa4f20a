#!/usr/bin/env python3
"""Generate the OM-LSTM goldens (tests/golden/om_lstm_*.npz) by importing the reference itself:

    python tests/golden/make_golden_om_lstm.py --reference PATH_OF_THE_REFERENCE_TREE

The reference's own LstmRL (rl/policy/lstm_rl.py) with [lstm_rl] with_om = true drives the reference's env (rvo2
substituted, like gen_lstm of make_golden_lstm.py) on the generated a5 and n10 scenes, for both of its value networks
(policy_lstm_interaction.config: ValueNetwork2, policy.config: ValueNetwork1), phase "train" with epsilon 0.  No tree ships
OM-LSTM weights: the network is the one configure() builds after torch.manual_seed(11), and no weight file is written; a
run's meta records every tensor's name, shape and SHA-256 and tests/om_lstm_cases.py rebuilds the network from the seed.

Per decision: the action, the 81 values, last_state [R, 61] (the rows sorted by decreasing distance with the maps
transform() built from the SORTED state), the maps predict() built (build_occupancy_maps is wrapped while the run lasts)
with the rows they were built from (the first action's next states, in the env's order), the sorted rows transform() built
its maps from, reward and info.

make_golden_om.py's two refusals hold here too: no file is written in which a coordinate of any (row, other) pair lies
within 1e-9 cells of a cell boundary (ebcsim.occupancy.boundary_margin), nor one in which any decision's top-2 gap is below
twice the value tolerance (TOL_FACTOR x the float32 error of the reference's own network against a float64 LstmModule
with its weights, measured on every forward of the run); the candidate test cases of a run are tried in turn.  Everything written is data."""
import argparse
import copy
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (A5, BIG, N10, RVO2_MODE, cfg_text, install_shims, jdump, save, scene_arrays,  # noqa: E402
                         write_tmp, info_code, parsed)
from make_golden_lstm import POLICY_CONFIGS, SEED  # noqa: E402
from make_golden_om import MARGIN, TOL_FACTOR, same_maps  # noqa: E402
from ebcsim import config as ebc_config  # noqa: E402
from ebcsim.lstm_rl import LstmModule  # noqa: E402
from ebcsim.occupancy import OccupancySpec, boundary_margin, occupancy_maps  # noqa: E402

# (scene tag, env config, overrides, candidate test cases): the first candidate that passes both refusals is taken
SCENES = [("a5", A5, None, (2, 7, 9, 10, 11, 3, 4, 5)),
          ("n10", BIG, N10, (1, 2, 3, 4, 5, 6))]


def run_once(text, pol_text, case):
    import torch
    from simulator.utils.test_utils import configure_env_policy_robot
    tmp, ptmp = write_tmp(text), write_tmp(pol_text)
    try:
        torch.manual_seed(SEED)
        env, pol, robot = configure_env_policy_robot(tmp, ptmp, None, phase="train", policy="lstm_rl")
    finally:
        os.unlink(tmp)
        os.unlink(ptmp)
    assert pol.with_om and pol.name == "LSTM-RL"
    pol.set_epsilon(0.0)
    spec = OccupancySpec(pol.cell_num, pol.cell_size, pol.om_channel_size)
    # the reference's forward builds float32 h0 / c0 whatever the module's dtype: the float64 copy is this package's
    # LstmModule (the same layers under the same names) on the reference's own state_dict
    m64 = LstmModule.from_state_dict(copy.deepcopy(pol.get_model().state_dict())).double().eval()
    err = {"values": 0.0, "calls": 0}

    def watch(module, inputs, output):
        with torch.no_grad():
            o64 = m64(inputs[0].double())
        assert o64.shape == output.shape
        err["values"] = max(err["values"], float((output.detach().double() - o64).abs().max()))
        err["calls"] += 1
    pol.get_model().register_forward_hook(watch)
    built = []
    inner = pol.build_occupancy_maps

    def wrapped(agent_states):
        om = inner(agent_states)
        built.append((np.array([[s.px, s.py, s.vx, s.vy, s.radius] for s in agent_states], dtype=np.float64), om.numpy().copy()))
        return om
    pol.build_occupancy_maps = wrapped
    ob, _ = env.reset("test", test_case=case, compute_local_map=False)
    init = scene_arrays(env)
    rec = dict(acts=[], vals=[], infos=[], rewards=[], last=[], om=[], om_ob=[], last_ob=[])
    margin = np.inf
    done = False
    while not done and len(rec["acts"]) < 200:
        del built[:]
        action = robot.act(ob, env=env)
        assert len(built) == 2, len(built)  # predict's maps (the first action's next states), then transform's (sorted)
        rec["acts"].append([action[0], action[1]])
        rec["vals"].append(list(pol.action_values))
        rec["last"].append(pol.last_state.numpy().astype(np.float32))
        rec["om_ob"].append(built[0][0])
        rec["om"].append(built[0][1])
        rec["last_ob"].append(built[1][0])
        assert (rec["last"][-1][:, 13:] == built[1][1]).all()
        for rows_, om_ in built:
            margin = min(margin, float(boundary_margin(rows_[None], None, spec).min()))
            same_maps(occupancy_maps(rows_[None], None, spec)[0], om_, spec)
        ob, _, reward, done, info = env.step(action, compute_local_map=False)
        rec["infos"].append(info_code(info))
        rec["rewards"].append(reward)
    assert err["calls"] == 81 * len(rec["acts"])
    v = np.sort(np.array(rec["vals"]), axis=1)
    gap = float(np.min(v[:, -1] - v[:, -2]))
    return env, pol, init, rec, spec, margin, gap, err["values"], len(ob)


def gen_runs(ref):
    RVO2_MODE["substitute"] = True
    for tag, pol_path in POLICY_CONFIGS:
        pol_text = cfg_text(os.path.join(ref, pol_path), {("lstm_rl", "with_om"): "true"})
        for scene, env_path, overrides, cases in SCENES:
            name = "om_lstm_%s_%s" % (tag, scene)
            text = cfg_text(os.path.join(ref, env_path), overrides)
            for case in cases:
                env, pol, init, rec, spec, margin, gap, e32, n_rows = run_once(text, pol_text, case)
                tol = TOL_FACTOR * e32
                print("  %s case %d: %d rows, %d decisions, final info code %d, top-2 gap %.3g, float32 error %.3g (tolerance "
                      "%.3g), closest boundary %.3g cells" % (name, case, n_rows, len(rec["acts"]), rec["infos"][-1], gap, e32,
                                                               tol, margin))
                if gap > 2 * tol and margin >= MARGIN:
                    break
            else:
                raise SystemExit("%s: no candidate case has its top-2 gap above twice the tolerance and every coordinate %g "
                                 "cells off the boundaries" % (name, MARGIN))
            params = ebc_config.params_from_config(parsed(text), parsed(pol_text), policy="om_lstm_rl")
            out = {("init_" + k): v for k, v in init.items()}
            out.update(action=np.array(rec["acts"]), values=np.array(rec["vals"]), info=np.array(rec["infos"]),
                       reward=np.array(rec["rewards"], float), last_state=np.stack(rec["last"]), om=np.stack(rec["om"]),
                       om_ob=np.stack(rec["om_ob"]), last_ob=np.stack(rec["last_ob"]),
                       action_space=np.array([[a[0], a[1]] for a in pol.action_space]),
                       params=jdump(ebc_config.params_to_dict(params)),
                       meta=jdump({"config": env_path, "config_text": text, "policy_config": pol_path, "policy_config_text": pol_text,
                                   "gamma": pol.gamma, "phase": "train", "seed_case": case, "torch_seed": SEED, "rows": n_rows,
                                   "cell_num": spec.cell_num, "cell_size": spec.cell_size, "channels": spec.channels,
                                   "input_dim": pol.input_dim(), "with_interaction_module": tag == "interaction",
                                   "state_dict": [[k, list(t.shape), hashlib.sha256(t.detach().numpy().tobytes()).hexdigest()]
                                                  for k, t in pol.get_model().state_dict().items()],
                                   "final_info": rec["infos"][-1], "top2_gap": gap, "float32_error": e32,
                                   "closest_boundary": margin}))
            save(name, **out)
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
    gen_runs(args.reference)


if __name__ == "__main__":
    main()
