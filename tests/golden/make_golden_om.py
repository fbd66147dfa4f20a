#!/usr/bin/env python3
"""Generate the OM-SARL goldens (tests/golden/om_cases.npz, tests/golden/om_sarl_*.npz) by importing the reference itself:

    python tests/golden/make_golden_om.py --reference PATH_OF_THE_REFERENCE_TREE

(a) om_cases.npz: the reference's own build_occupancy_maps (rl/policy/multi_human_rl.py:156-227) on constructed float64
states — random ones (2-18 rows, standing rows, coincident pairs, rows inside and outside the grid), and by kind:
coincident groups, standing rows only, the four sign combinations of a zero velocity, rows far outside the grid, R = 2 —
for every channel count and every (cell_num, cell_size) of SPECS.

(b) om_sarl_*.npz: the reference's own SARL with with_om = true driving the reference's env (rvo2 substituted, like
gen_sarl of make_golden.py) on the generated a5 and n10 scenes of SARL_RUNS, phase "train" with epsilon 0.  No tree
ships OM weights: the network is the one configure() builds after torch.manual_seed(11), and no weight file is written;
a run's meta records every tensor's name, shape and SHA-256 and tests/om_cases.py rebuilds the network from the seed.
Per decision: the action, the 81 values, last_state [R, T + W], the maps predict() built (build_occupancy_maps is wrapped
while the run lasts) and the rows they were built from, reward and info.

The product states the reference's arctan2 / cos / sin frame algebraically; the two agree except for a coordinate that
lies exactly on a cell boundary.  The generator therefore refuses to write a file in which a coordinate of any
(row, other) pair lies within 1e-9 cells of a boundary (ebcsim.occupancy.boundary_margin; excepted, because exact in both
forms: coincident pairs, and a standing row's axis along which the occupant's offset is exactly 0: the wall rows of the
n10 scene stand in axis-aligned pairs), and it asserts that the product's maps of every recorded state hold the
tolerance of tests/om_cases.py against the reference's.  Everything written is data."""
import argparse
import copy
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (A5, BIG, N10, P1, RVO2_MODE, SARL_RUNS, cfg_text, install_shims, jdump, save,  # noqa: E402
                         scene_arrays, write_tmp, info_code, parsed)
from ebcsim import config as ebc_config  # noqa: E402
from ebcsim.occupancy import OccupancySpec, boundary_margin, occupancy_maps  # noqa: E402

SEED = 11
TOL_FACTOR = 8
MARGIN = 1e-9
SPECS = [(4, 1.0), (3, 0.5), (5, 0.7), (8, 1.0)]
KINDS = ["random", "coincident", "standing", "zero_sign", "far", "two_rows"]
RANDOM_PER_COMBO = 25
R_MAX = 18
# (name, env config, overrides, policy config, om_channel_size, candidate test cases)
# the first candidate whose smallest top-2 gap exceeds twice the tolerance is taken.  An untrained network's values lie
# close together: cases 2-6 and 8 of the a5 scene have decisions 2e-7 to 7e-7 apart (tolerance 6e-7), case 7 has 3.9e-6.
RUNS = [("om_sarl_a5_c3", A5, None, P1, 3, (7, 9, 10, 11)),
        ("om_sarl_n10_c3", BIG, N10, SARL_RUNS[1][3], 3, (1, 2, 3, 4)),
        ("om_sarl_n10_c1", BIG, N10, P1, 1, (2, 1, 3, 4))]
assert SARL_RUNS[0][1] == A5 and SARL_RUNS[1][1] == BIG and SARL_RUNS[1][2] == N10


def same_maps(got, want, spec):
    """The tolerance of tests/om_cases.py: occupancy equal, a mean velocity within one float32 spacing + 1e-12."""
    col = np.arange(spec.width) % spec.channels
    vel = np.zeros(spec.width, bool) if spec.channels == 1 else (col >= spec.channels - 2)
    assert (got[:, ~vel] == want[:, ~vel]).all(), "an occupant falls into another cell than the reference's"
    d = np.abs(got[:, vel].astype(np.float64) - want[:, vel].astype(np.float64))
    assert (d <= np.spacing(np.abs(want[:, vel])).astype(np.float64) + 1e-12).all(), float(d.max())


def constructed_state(rs, kind):
    """[R, 5] float64 (px, py, vx, vy, radius)."""
    R = 2 if kind == "two_rows" else int(rs.randint(2, R_MAX + 1))
    ob = np.zeros((R, 5))
    ob[:, :2] = rs.uniform(-3.0, 3.0, (R, 2))
    ob[:, 2:4] = rs.normal(0.0, 0.8, (R, 2))
    ob[:, 4] = 0.3
    if kind == "random":
        still = rs.permutation(R)[:rs.randint(0, min(8, R) + 1)]
        ob[still, 2:4] = 0.0
        for _ in range(rs.randint(0, 3)):
            i, j = rs.permutation(R)[:2]
            ob[j, :2] = ob[i, :2]
    elif kind == "coincident":
        group = rs.permutation(R)[:max(2, R // 2)]
        ob[group, :2] = ob[group[0], :2]
    elif kind == "standing":
        ob[:, 2:4] = 0.0
    elif kind == "zero_sign":
        signs = [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]
        for r in range(R):
            if r < 4 or rs.uniform() < 0.3:
                ob[r, 2:4] = signs[r % 4]
    elif kind == "far":
        ob[:, :2] *= 100.0
        ob[rs.randint(R), :2] = (1e6, -1e6)
    return ob


def gen_cases(ref):
    from rl.policy.sarl import SARL
    from simulator.utils.state import ObservableState
    rs = np.random.RandomState(20261018)
    pol = SARL()
    obs, rows, spec_rows, kinds, maps, offsets = [], [], [], [], [], [0]
    for cell_num, cell_size in SPECS:
        for channels in (1, 2, 3):
            spec = OccupancySpec(cell_num, cell_size, channels)
            pol.cell_num, pol.cell_size, pol.om_channel_size = cell_num, cell_size, channels
            for kind in ["random"] * RANDOM_PER_COMBO + KINDS[1:]:
                while True:
                    ob = constructed_state(rs, kind)
                    if float(boundary_margin(ob[None], None, spec).min()) >= MARGIN:
                        break
                states = [ObservableState(*[float(x) for x in row]) for row in ob]
                om = pol.build_occupancy_maps(states).numpy()
                same_maps(occupancy_maps(ob[None], None, spec)[0], om, spec)
                assert om.dtype == np.float32 and om.shape == (len(ob), spec.width)
                pad = np.full((R_MAX, 5), np.nan)
                pad[:len(ob)] = ob
                obs.append(pad)
                rows.append(len(ob))
                spec_rows.append((cell_num, cell_size, channels))
                kinds.append(KINDS.index(kind))
                maps.append(om.reshape(-1))
                offsets.append(offsets[-1] + om.size)
    save("om_cases", ob=np.stack(obs), rows=np.array(rows, np.int64), cell_num=np.array([s[0] for s in spec_rows], np.int64),
         cell_size=np.array([s[1] for s in spec_rows]), channels=np.array([s[2] for s in spec_rows], np.int64),
         kind=np.array(kinds, np.int64), maps=np.concatenate(maps), offsets=np.array(offsets, np.int64),
         meta=jdump({"kinds": KINDS, "margin": MARGIN, "specs": SPECS, "random_per_combo": RANDOM_PER_COMBO}))
    print("  om_cases: %d states, %d float32 values" % (len(rows), offsets[-1]))


def run_once(ref, text, pol_text, case):
    import torch
    from simulator.utils.test_utils import configure_env_policy_robot
    tmp, ptmp = write_tmp(text), write_tmp(pol_text)
    try:
        torch.manual_seed(SEED)
        env, pol, robot = configure_env_policy_robot(tmp, ptmp, None, phase="train", policy="sarl")
    finally:
        os.unlink(tmp)
        os.unlink(ptmp)
    assert pol.with_om and pol.name == "OM-SARL"
    pol.set_epsilon(0.0)
    spec = OccupancySpec(pol.cell_num, pol.cell_size, pol.om_channel_size)
    m64 = copy.deepcopy(pol.get_model()).double()
    err = {"values": 0.0, "calls": 0}

    def watch(module, inputs, output):
        with torch.no_grad():
            o64 = m64(inputs[0].double())
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
    rec = dict(acts=[], vals=[], infos=[], rewards=[], last=[], om=[], om_ob=[])
    margin = np.inf
    done = False
    while not done and len(rec["acts"]) < 200:
        del built[:]
        action = robot.act(ob, env=env)
        assert len(built) == 2, len(built)  # predict's maps (the first action's next states), then transform's
        rec["acts"].append([action[0], action[1]])
        rec["vals"].append(list(pol.action_values))
        rec["last"].append(pol.last_state.numpy().astype(np.float32))
        rec["om_ob"].append(built[0][0])
        rec["om"].append(built[0][1])
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
    for name, env_path, overrides, pol_path, channels, cases in RUNS:
        text = cfg_text(os.path.join(ref, env_path), overrides)
        pol_text = cfg_text(os.path.join(ref, pol_path), {("sarl", "with_om"): "true", ("om", "om_channel_size"): channels})
        for case in cases:
            env, pol, init, rec, spec, margin, gap, e32, n_rows = run_once(ref, text, pol_text, case)
            tol = TOL_FACTOR * e32
            print("  %s case %d: %d rows, %d decisions, final info code %d, top-2 gap %.3g, float32 error %.3g (tolerance %.3g), "
                  "closest boundary %.3g cells" % (name, case, n_rows, len(rec["acts"]), rec["infos"][-1], gap, e32, tol, margin))
            if gap > 2 * tol and margin >= MARGIN:
                break
        else:
            raise SystemExit("%s: no candidate case has its top-2 gap above twice the tolerance and every coordinate %g cells "
                             "off the boundaries" % (name, MARGIN))
        params = ebc_config.params_from_config(parsed(text), parsed(pol_text))
        out = {("init_" + k): v for k, v in init.items()}
        out.update(action=np.array(rec["acts"]), values=np.array(rec["vals"]), info=np.array(rec["infos"]),
                   reward=np.array(rec["rewards"], float), last_state=np.stack(rec["last"]), om=np.stack(rec["om"]),
                   om_ob=np.stack(rec["om_ob"]),
                   action_space=np.array([[a[0], a[1]] for a in pol.action_space]),
                   params=jdump(ebc_config.params_to_dict(params)),
                   meta=jdump({"config": env_path, "config_text": text, "policy_config": pol_path, "policy_config_text": pol_text,
                               "gamma": pol.gamma, "phase": "train", "seed_case": case, "torch_seed": SEED, "rows": n_rows,
                               "cell_num": spec.cell_num, "cell_size": spec.cell_size, "channels": spec.channels,
                               "input_dim": pol.input_dim(), "with_agent_type": bool(pol.with_agent_type),
                               "state_dict": [[k, list(t.shape), hashlib.sha256(t.detach().numpy().tobytes()).hexdigest()]
                                              for k, t in pol.get_model().state_dict().items()],
                               "final_info": rec["infos"][-1], "top2_gap": gap, "float32_error": e32,
                               "closest_boundary": margin, "with_global_state": True}))
        save(name, **out)
    RVO2_MODE["substitute"] = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--only", choices=["cases", "runs"], default=None)
    args = ap.parse_args()
    args.reference = os.path.abspath(args.reference)
    install_shims()
    sys.path.insert(0, args.reference)
    os.chdir(args.reference)  # the reference resolves config paths relative to its root
    import logging
    logging.disable(logging.CRITICAL)
    if args.only in (None, "cases"):
        gen_cases(args.reference)
    if args.only in (None, "runs"):
        gen_runs(args.reference)


if __name__ == "__main__":
    main()
