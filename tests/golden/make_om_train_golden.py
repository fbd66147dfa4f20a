#!/usr/bin/env python3
"""Generate tests/golden/om_train_states.npz by importing the reference itself:

    python tests/golden/make_om_train_golden.py --reference PATH_OF_THE_REFERENCE_TREE

The state OM-SARL stores for training is the reference's SARL.transform(state) with with_om = true
(rl/policy/multi_human_rl.py:128-149): [rotate(state) | build_occupancy_maps(state.agent_states)].  This records it for
constructed JointStates, with the inputs that produced it: PER_COMBO states for every combination of the two row widths
(with_agent_type), channels 1, 2, 3 and cell_num 1 and 4, the kinematics alternating; 1 to 6 rows in turn; by kind: random
rows, standing rows with vx = +0 and vx = -0, coincident rows.

One row.  build_occupancy_maps of a single agent asks np.concatenate for the rows of its empty list of others and raises
ValueError: the reference cannot transform such a state with maps at all.  The generator tries it, records that it
raised (meta "one_row_raises") and stores for that state what the reference can give: rotate(state) of its transform
without maps, and no map columns (the state's width is T).  The product gives a lone row an empty map.

The product states the reference's arctan2 / cos / sin frame algebraically; the two agree except for a coordinate that
lies on a cell boundary to within float64 rounding.  A state with a non-coincident pair within MARGIN cells of a boundary
(tests/om_cases.py: MARGIN; ebcsim.occupancy.boundary_margin) is drawn again until every slot has its state, and the
number of redraws is stored.  Everything written is data."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import install_shims, jdump, save  # noqa: E402
from ebcsim.occupancy import OccupancySpec, boundary_margin  # noqa: E402
from om_cases import MARGIN  # noqa: E402

PER_COMBO = 6
R_MAX = 6
CELL_SIZE = {1: 3.0, 4: 1.0}
KINDS = ["random", "standing", "coincident"]


def constructed(rs, R, kind):
    """(robot [9] FullState order, ob [R, 5] (px, py, vx, vy, radius), agent types [R]) in float64."""
    robot = np.zeros(9)
    robot[:2] = rs.uniform(-4.0, 4.0, 2)
    robot[2:4] = rs.normal(0.0, 0.6, 2)
    robot[4] = 0.3
    robot[5:7] = rs.uniform(-4.0, 4.0, 2)
    robot[7] = rs.uniform(0.5, 1.5)
    robot[8] = rs.uniform(-np.pi, np.pi)
    ob = np.zeros((R, 5))
    ob[:, :2] = rs.uniform(-2.0, 2.0, (R, 2))
    ob[:, 2:4] = rs.normal(0.0, 0.8, (R, 2))
    ob[:, 4] = rs.uniform(0.2, 0.5, R)
    if kind == "standing":  # vx = +0 and vx = -0 in turn, vy of either sign
        signs = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
        for r in range(R):
            if r < 2 or rs.uniform() < 0.5:
                ob[r, 2:4] = signs[(r + R) % 4]
    elif kind == "coincident" and R > 1:
        group = rs.permutation(R)[:max(2, R // 2)]
        ob[group, :2] = ob[group[0], :2]
    return robot, ob, rs.randint(0, 4, R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    install_shims()
    sys.path.insert(0, ref)
    os.chdir(ref)
    import logging
    logging.disable(logging.CRITICAL)
    import torch
    from rl.policy.sarl import SARL
    from simulator.utils.state import FullState, JointState, ObservableState

    rs = np.random.RandomState(20261020)
    rec = dict(robot=[], ob=[], types=[], rows=[], T=[], unicycle=[], cell_num=[], cell_size=[], channels=[], kind=[], state=[],
               offsets=[0])
    redrawn, one_row_raises, slot = 0, 0, 0
    for with_type in (False, True):
        for channels in (1, 2, 3):
            for cell_num in (1, 4):
                spec = OccupancySpec(cell_num, CELL_SIZE[cell_num], channels)
                for i in range(PER_COMBO):
                    R, kind, unicycle = 1 + slot % R_MAX, KINDS[(slot // R_MAX + i) % len(KINDS)], bool((slot // 2) % 2)
                    slot += 1
                    while True:
                        robot, ob, types = constructed(rs, R, kind)
                        if float(boundary_margin(ob[None], None, spec).min()) >= MARGIN:
                            break
                        redrawn += 1
                    pol = SARL()
                    pol.device = torch.device("cpu")
                    pol.kinematics = "unicycle" if unicycle else "holonomic"
                    pol.with_agent_type, pol.agent_type_state_dim = with_type, 4
                    pol.with_om, pol.cell_num, pol.cell_size, pol.om_channel_size = True, spec.cell_num, spec.cell_size, spec.channels
                    state = JointState(FullState(*[float(x) for x in robot]),
                                       [ObservableState(*[float(x) for x in row], obj_type=int(t)) for row, t in zip(ob, types)])
                    T = 17 if with_type else 13
                    try:
                        out = pol.transform(state).numpy()
                        assert out.shape == (R, T + spec.width), out.shape
                    except ValueError:
                        assert R == 1, "only a lone row may fail (np.concatenate of no others)"
                        one_row_raises += 1
                        pol.with_om = False
                        out = pol.transform(state).numpy()
                        assert out.shape == (1, T), out.shape
                    assert out.dtype == np.float32
                    pad = np.full((R_MAX, 5), np.nan)
                    pad[:R] = ob
                    tp = np.zeros(R_MAX, np.int64)
                    tp[:R] = types
                    rec["robot"].append(robot)
                    rec["ob"].append(pad)
                    rec["types"].append(tp)
                    rec["rows"].append(R)
                    rec["T"].append(T)
                    rec["unicycle"].append(int(unicycle))
                    rec["cell_num"].append(spec.cell_num)
                    rec["cell_size"].append(spec.cell_size)
                    rec["channels"].append(spec.channels)
                    rec["kind"].append(KINDS.index(kind))
                    rec["state"].append(out.reshape(-1))
                    rec["offsets"].append(rec["offsets"][-1] + out.size)
    n = len(rec["rows"])
    save("om_train_states", robot=np.stack(rec["robot"]), ob=np.stack(rec["ob"]), types=np.stack(rec["types"]),
         rows=np.array(rec["rows"], np.int64), T=np.array(rec["T"], np.int64), unicycle=np.array(rec["unicycle"], np.int64),
         cell_num=np.array(rec["cell_num"], np.int64), cell_size=np.array(rec["cell_size"]),
         channels=np.array(rec["channels"], np.int64), kind=np.array(rec["kind"], np.int64), state=np.concatenate(rec["state"]),
         offsets=np.array(rec["offsets"], np.int64), redrawn=np.array(redrawn, np.int64),
         meta=jdump({"kinds": KINDS, "margin": MARGIN, "per_combo": PER_COMBO, "states": n, "redrawn": redrawn,
                     "one_row_raises": one_row_raises, "cell_size": {str(k): v for k, v in CELL_SIZE.items()}}))
    print("  om_train_states: %d states, %d redrawn, %d lone rows the reference's maps raise on" % (n, redrawn, one_row_raises))


if __name__ == "__main__":
    main()
