#!/usr/bin/env python3
"""Generate tests/golden/scenes_crowd_rules.npz and tests/golden/traj_mix20_orcasub.npz by importing the reference itself:

    python tests/golden/make_golden_crowd_rules.py --reference PATH_OF_THE_REFERENCE_TREE

The crowd rules are the adult rules `mixed`, `mixed_20` and `one_static` of generate_random_adult_position
(simulator/scene/scene_generator.py:523-589, with generate_static_adults :459-490 and generate_dynamic_adults :492-501).

scenes_crowd_rules.npz: the reference's own scenes under each rule, env.reset("test", scene_number=seed) through the
import shims of make_golden.py.  Set s holds the scenes of one config: meta_s (config text, rule, randomized), seed_s,
and the arrays of scene_arrays end to end as KEY_s with count_s humans and n_static_s rows per scene (grid_s: bits):
  mixed       seeds 3000..3095  every branch: standing 0 (3031) .. 5, walking 1 .. 5 (4 at 3038, 5 at 3050)
  mixed_20    seeds 3000..3064  every number of standing adults 0 (3008) .. 19 (3000)
  one_static  seeds 3000, 3001
  mixed_20    seeds 3000..3064 with randomize_attributes = true, three bicycles, two children, two circles and two
              walls; the value ranges are those of adults_8_bikes_8_child_8_static_3_35_sec_new_reward.config
All from env_adults_5.config with the keys below overridden.  `mixed` overwrites the generator's adult_num with the
number it drew (:537); it is set back to 5 before every reset so that no case depends on the one before it.

traj_mix20_orcasub.npz: one episode on mixed_20 at seed 3007 (14 standing adults, 6 walking) with a scripted robot
and the oracle-substituted rvo2 of the `_orcasub` fixtures, 40 steps or to the terminal step.  A standing adult is an
ORCA human whose goal is its position: its preferred velocity is zero and the others still push it around.

Everything written is data."""
import argparse
import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import A5, BIG, P1, cfg_text, jdump, make_env, run_trajectory, scene_arrays, install_shims  # noqa: E402

TRAJ = "traj_mix20_orcasub"
TRAJ_SEED = 3007
RANGES = {(sec, key): None for sec in ("adults", "bicycles", "children")
          for key in ("v_pref_min", "v_pref_max", "radius_min", "radius_max")}


def rule_overrides(rule, adult_num):
    return {("sim", "train_val_sim_adult"): rule, ("sim", "test_sim_adult"): rule, ("sim", "adult_num"): adult_num}


def randomized_overrides(ref):
    """mixed_20 with random attributes, bicycles, children and a map: the ranges are the shipped ones of BIG."""
    import configparser
    big = configparser.RawConfigParser()
    big.read(os.path.join(ref, BIG))
    ov = rule_overrides("mixed_20", 20)
    for sec, key in RANGES:
        ov[(sec, key)] = big.get(sec, key)
    ov.update({("env", "randomize_attributes"): "true", ("sim", "bicycle_num"): 3, ("sim", "children_num"): 2,
               ("sim", "train_val_sim_children"): "square_crossing", ("sim", "test_sim_children"): "square_crossing",
               ("map", "num_circles"): 2, ("map", "num_walls"): 2,
               ("children", "visible"): "true", ("children", "policy"): "orca", ("children", "sensor"): "coordinates",
               ("children", "radius"): 0.15, ("children", "v_pref"): 0.5})
    return ov


def gen_scenes(ref):
    pol = os.path.join(ref, P1)
    sets = [("mixed", rule_overrides("mixed", 5), range(3000, 3096), False),
            ("mixed_20", rule_overrides("mixed_20", 20), range(3000, 3065), False),
            ("one_static", rule_overrides("one_static", 2), (3000, 3001), False),
            ("mixed_20", randomized_overrides(ref), range(3000, 3065), True)]
    out = {}
    for s, (rule, ov, seeds, randomized) in enumerate(sets):
        text = cfg_text(os.path.join(ref, A5), ov)
        env, _, _ = make_env(ref, text, pol)
        rows = []
        for seed in seeds:
            env.scene.adult_num = int(ov[("sim", "adult_num")])
            env.reset("test", compute_local_map=False, scene_number=seed)
            rows.append(scene_arrays(env))
        # one set = one config: the scenes' arrays end to end, `count` humans and `n_static` rows per scene
        out["meta_%d" % s] = jdump({"config": A5, "rule": rule, "randomized": randomized, "config_text": text})
        out["seed_%d" % s] = np.array(list(seeds), np.int64)
        out["count_%d" % s] = np.array([len(r["px"]) for r in rows], np.int32)
        out["n_static_%d" % s] = np.array([len(r["static"]) for r in rows], np.int32)
        for key in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type", "static"):
            out["%s_%d" % (key, s)] = np.concatenate([r[key] for r in rows])
        out["grid_%d" % s] = np.packbits(np.stack([r["grid"] for r in rows]), axis=2)  # 1 = occupied, as in scenes.npz
        out["robot_%d" % s] = np.stack([r["robot"] for r in rows])
        standing = [int(((r["px"] == r["gx"]) & (r["py"] == r["gy"])).sum()) for r in rows]
        adults = [int((r["type"] == 0).sum()) for r in rows]
        print("  %-10s randomized=%-5s %3d scenes, adults %d..%d, standing %d..%d" % (
            rule, randomized, len(rows), min(adults), max(adults), min(standing), max(standing)))
    out["n_sets"] = np.array(len(sets))
    path = os.path.join(HERE, "scenes_crowd_rules.npz")
    np.savez_compressed(path, **out)
    print("wrote scenes_crowd_rules.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


def gen_trajectory(ref):
    # test case c of phase "test" is seed 1000 + c (simulator/env.py:153-158)
    run_trajectory(ref, TRAJ, A5, rule_overrides("mixed_20", 20), P1, "scripted", 40, TRAJ_SEED - 1000, orca=True,
                   lookahead_every=20, stop_when_done=True)
    path = os.path.join(HERE, TRAJ + ".npz")
    z = dict(np.load(path, allow_pickle=False))
    standing = int(((z["init_px"] == z["init_gx"]) & (z["init_py"] == z["init_gy"])).sum())
    assert len(z["init_px"]) == 20 and standing == 14, (len(z["init_px"]), standing)
    meta = json.loads(str(z["meta"]))
    meta["seed"], meta["standing"] = TRAJ_SEED, standing
    z["meta"] = jdump(meta)
    np.savez_compressed(path, **z)
    print("wrote %s.npz %.1f KB: %d steps, final info %d" % (TRAJ, os.path.getsize(path) / 1024.0, len(z["action"]),
                                                              meta["final_info"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--only", choices=("scenes", "trajectory"), default=None)
    args = ap.parse_args()
    install_shims()
    sys.path.insert(0, args.reference)
    os.chdir(args.reference)  # the reference resolves config paths relative to its root
    logging.disable(logging.CRITICAL)
    if args.only in (None, "scenes"):
        gen_scenes(args.reference)
    if args.only in (None, "trajectory"):
        gen_trajectory(args.reference)


if __name__ == "__main__":
    main()
