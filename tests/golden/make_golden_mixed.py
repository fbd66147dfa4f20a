#!/usr/bin/env python3
"""Generate tests/golden/traj_mixed_a3b3c2.npz by importing the reference itself:

    python tests/golden/make_golden_mixed.py --reference PATH_OF_THE_REFERENCE_TREE

The reference's own env runs a scene of three adults, three bicycles and two children in which `[bicycles] policy =
linear` while adults and children stay on `orca` (every entity type carries its own policy: simulator/agents/agent.py:19,
simulator/env.py:392-405), with scripted robot actions, through run_trajectory of make_golden.py and its import shims.
rvo2 is the oracle-substituted one of the `_orcasub` fixtures: the run pins the reference's ORCHESTRATION of a mixed scene
(who is whose neighbour with which velocity, the order of the updates), not ORCA's arithmetic.  The table of policies per
type goes into the fixture's meta.  Everything written is data."""
import argparse
import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import BIG, P1, install_shims, jdump, run_trajectory  # noqa: E402

NAME = "traj_mixed_a3b3c2"
TABLE = {"adults": "orca", "bicycles": "linear", "children": "orca"}
OVERRIDES = {("sim", "adult_num"): 3, ("sim", "bicycle_num"): 3, ("sim", "children_num"): 2}
OVERRIDES.update({(section, "policy"): policy for section, policy in TABLE.items()})
STEPS, CASE = 40, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    install_shims()
    sys.path.insert(0, args.reference)
    os.chdir(args.reference)  # the reference resolves config paths relative to its root
    logging.disable(logging.CRITICAL)
    run_trajectory(args.reference, NAME, BIG, OVERRIDES, P1, "scripted", STEPS, CASE, orca=True, lookahead_every=20)
    path = os.path.join(HERE, NAME + ".npz")
    z = dict(np.load(path, allow_pickle=False))
    types = sorted(set(int(t) for t in z["init_type"]))
    assert types == [0, 1, 2] and len(z["init_type"]) == 8, types
    meta = json.loads(str(z["meta"]))
    meta["human_policy"] = "by_type"
    meta["human_policies"] = [TABLE["adults"], TABLE["bicycles"], TABLE["children"]]
    z["meta"] = jdump(meta)
    np.savez_compressed(path, **z)
    print("wrote %s.npz %.1f KB" % (NAME, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
