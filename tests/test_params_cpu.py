"""What the runs of tests/params_cases.py are worth, asserted from the oracle alone (no GPU): each of them differs from the
same run at the default time_step / ORCA horizon / safety space, every env restarts inside it, the info codes 0-4 and the
time-out all occur, the accumulated clock passes time_limit where a plain product would not say so, and
ebcsim.config.params_from_config rebuilds the parameters of the three fixtures that pin the oracle itself off the default.
tests/test_params_gpu.py holds the kernels to these very runs.  The table goes to profiles/param_coverage.txt between its
BEGIN / END markers; the figures measured on the device stand in a section of their own, which the GPU test writes."""
import configparser
import json
import os

import numpy as np
import pytest

import params_cases as pc
from ebcsim import _abi, config as ebc_config
from helpers import (ORCA_HUMAN_CASES, ORCA_MOVED_SETS, ORCA_PARAM_SETS, config_text_of, load, orca_case_id, orca_human_batch,
                     orca_reference, params_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "param_coverage.txt")
HUMANS = {"linear": _abi.HUMAN_LINEAR, "orca": _abi.HUMAN_ORCA}
STEP_RUNS = [(ps, kin, h) for ps in pc.SETS for kin in pc.KINEMATICS for h in HUMANS]
STEP_K_RUNS = [(ps, form) for ps in pc.SETS for form in pc.STEP_K_FORMS]
CODES = (_abi.INFO_NOTHING, _abi.INFO_DANGER, _abi.INFO_REACH_GOAL, _abi.INFO_COLLISION_OBSTACLE, _abi.INFO_COLLISION_ADULT,
         _abi.INFO_TIMEOUT)


def _differs(a, b, exists=None):
    d = a != b
    return int((d if exists is None else d & exists).sum())


def _humans_exist(state):
    return np.arange(pc.N)[None, :] < state["n_humans"][:, None]


@pytest.mark.parametrize("ps,kin,humans", STEP_RUNS, ids=lambda v: str(v))
def test_step_runs_differ_from_the_default_fields(ps, kin, humans):
    """State after step 1.  Positions move with time_step: against the same run at 0.25 every human that moves and every
    robot that moves stands elsewhere.  Under "all" with ORCA humans the velocities move with the horizon and the safety
    space: against the same run at time_step 0.1 with horizon 5 and safety space 0."""
    ref = pc.step_reference(ps, kin, HUMANS[humans])
    moved = ref["state"][0]
    plain = pc.step_walk(pc.case_params(ps, kin, **pc.default_fields(ps, ("time_step",))), kin, HUMANS[humans], steps=1)["state"][0]
    live = ~ref["out"][0]["done"].astype(bool)  # an env that ended at step 1 holds its pool scene in both runs
    assert live.sum() >= pc.E // 2
    exists = _humans_exist(moved) & live[:, None]
    walking = exists & ((moved["vx"] != 0) | (moved["vy"] != 0))
    assert walking.sum() >= exists.sum() // 2
    assert ((moved["px"] != plain["px"]) | (moved["py"] != plain["py"]))[walking].all()
    driven = live & (np.abs(pc.robot_actions(kin)[0][:, 0]) > 0)
    assert driven.sum() >= pc.E // 3
    assert ((moved["robot"][:, 0] != plain["robot"][:, 0]) | (moved["robot"][:, 1] != plain["robot"][:, 1]))[driven].all()
    if ps == "all" and humans == "orca":
        plain = pc.step_walk(pc.case_params(ps, kin, **pc.default_fields(ps, pc.FIELDS[1:])), kin, HUMANS[humans], steps=1)["state"][0]
        changed = _differs(moved["vx"], plain["vx"], exists) + _differs(moved["vy"], plain["vy"], exists)
        assert 10 * changed >= 2 * exists.sum(), (changed, int(exists.sum()))


@pytest.mark.parametrize("ps,kin,humans", STEP_RUNS, ids=lambda v: str(v))
def test_step_runs_restart_every_env_at_the_clock_s_own_step(ps, kin, humans):
    """Every env restarts inside the window; a time-out comes at the first step that STARTS with the accumulated clock at
    or past time_limit (env.py compares before it advances the clock): the 14th step at 0.1, after 13 additions; the
    fourth at 0.5, which starts at 1.5."""
    ref = pc.step_reference(ps, kin, HUMANS[humans])
    done = np.stack([o["done"] for o in ref["out"]]).astype(bool)
    info = np.stack([o["info"] for o in ref["out"]])
    assert done.any(0).all(), "envs that never restart: %s" % np.flatnonzero(~done.any(0)).tolist()
    dt = ORCA_PARAM_SETS[ps][2]
    clock, want = 0.0, 0
    while clock < pc.TIME_LIMIT:
        clock, want = clock + dt, want + 1
    want += 1
    assert want == {0.1: 14, 0.5: 4}[dt]
    age = np.zeros(pc.E, int)
    for t in range(pc.STEPS):
        age += 1
        timed_out = info[t] == _abi.INFO_TIMEOUT
        assert (age[timed_out] == want).all() and (age[~done[t]] < want).all(), (t, age, info[t])
        age[done[t]] = 0
    assert (info == _abi.INFO_TIMEOUT).any()


def test_every_info_code_occurs():
    seen = _code_counts()
    for code in CODES:
        assert sum(c.get(code, 0) for c in seen.values()) >= 1, (code, seen)
    for ps in pc.SETS:  # and in the runs of each set taken alone
        for code in CODES:
            assert sum(c.get(code, 0) for k, c in seen.items() if k[0] == ps) >= 1, (ps, code)


def _code_counts():
    seen = {}
    for ps, kin, humans in STEP_RUNS:
        info = np.stack([o["info"] for o in pc.step_reference(ps, kin, HUMANS[humans])["out"]])
        seen[ps, "step " + humans, kin] = dict(zip(*[x.tolist() for x in np.unique(info, return_counts=True)]))
    for ps, form in STEP_K_RUNS:
        info = pc.step_k_reference(ps, form)["out"]["info"]
        seen[ps, "step_k " + form[0] + (" sim" if form[2] else ""), form[1]] = dict(
            zip(*[x.tolist() for x in np.unique(info, return_counts=True)]))
    return seen


@pytest.mark.parametrize("ps,form", STEP_K_RUNS, ids=lambda v: v if isinstance(v, str) else pc.form_id(v))
def test_step_k_runs_restart_and_differ_from_the_default_fields(ps, form):
    robot, kin, sim = form
    ref = pc.step_k_reference(ps, form)
    assert ref["out"]["done"].astype(bool).any(0).all()
    plain = pc.step_k_walk(pc.case_params(ps, kin, **pc.default_fields(ps)), robot, kin, sim)
    assert (ref["out"]["reward"][0] != plain["out"]["reward"][0]).any()
    if robot == "external":  # the same walk as the per-step ORCA run
        step = pc.step_reference(ps, kin, _abi.HUMAN_ORCA)
        np.testing.assert_array_equal(ref["out"]["reward"], np.stack([o["reward"] for o in step["out"]]))
    if robot == "orca":  # the robot's own safety space is never the handle's (0.1 under "all", else 0)
        assert pc.ROBOT_SAFETY not in (0.0, ORCA_PARAM_SETS[ps][4])


def test_dagger_window_restarts_and_its_expert_sees_the_fields():
    """Every env of the DAgger case restarts inside its 8 steps, and the expert's first labels under "all" are not those
    under the default fields."""
    from oracle import oracle
    p, batch, pool, sd, mask = pc.dagger_setup()
    assert (p.time_step, p.orca_time_horizon, p.orca_safety_space) == (0.1, 2.0, 0.1) and mask.any() and not mask.all()
    o = oracle.OracleEnv(p, batch.n, batch.N, batch.S)
    o.reset(batch)
    moved = o.robot_orca(pc.DAGGER["safety"])
    out = o.step_k(pc.DAGGER["K"], ("done",), flags=pc.AUTO, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA,
                   robot_safety_space=pc.DAGGER["safety"])
    assert out["done"].astype(bool).any(0).all()
    for k, v in zip(pc.FIELDS, ORCA_PARAM_SETS["default"][2:]):
        setattr(p, k, v)
    o = oracle.OracleEnv(p, batch.n, batch.N, batch.S)
    o.reset(batch)
    assert 10 * int((o.robot_orca(pc.DAGGER["safety"]) != moved).any(1).sum()) >= batch.n


def test_il_and_evaluate_walks_end_episodes():
    il = pc.il_walk()
    stored = np.isin(il["info"], [_abi.INFO_REACH_GOAL, _abi.INFO_COLLISION_ADULT, _abi.INFO_COLLISION_BICYCLE,
                                  _abi.INFO_COLLISION_CHILD, _abi.INFO_COLLISION_OBSTACLE])
    assert stored.sum() >= pc.IL["E"] // 2 and (il["info"] == _abi.INFO_TIMEOUT).any()
    p, out = pc.eval_walk()
    tally = pc.eval_tally(p, out)
    assert tally["success"] >= 2 and tally["danger_steps"] >= 1 and 0 < tally["avg_nav_time"] < p.time_limit


FIXTURES = ["traj_a5_linear_dt01", "traj_unicycle_dt05", "traj_a3b3s2_dt01_orcasub"]


@pytest.mark.parametrize("name", FIXTURES)
def test_params_from_config_rebuilds_the_fixture_s_parameters(name):
    """The config text the fixture ran with plus the attributes recorded in its meta give its `params`, field by field."""
    z = load(name)
    meta = json.loads(str(z["meta"]))
    cfg = configparser.RawConfigParser()
    cfg.read_string(config_text_of(meta))
    pol = configparser.RawConfigParser()
    pol.read_string(json.loads(open(os.path.join(ROOT, "tests", "golden", "sarl_configs.json")).read())
                    ["sarl_a5_baseline"]["policy_config_text"])  # configs/test_configs/test_policy_configs/policy.config
    got = ebc_config.params_to_dict(ebc_config.params_from_config(cfg, pol, robot_kinematics=meta["kinematics"],
                                                                  human_orca=meta.get("human_orca")))
    want = ebc_config.params_to_dict(params_of(z))
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    moved = {"traj_a5_linear_dt01": (0.1, 5.0, 0.0), "traj_unicycle_dt05": (0.5, 5.0, 0.0),
             "traj_a3b3s2_dt01_orcasub": (0.1, 2.0, 0.1)}[name]
    assert (want["time_step"], want["orca_time_horizon"], want["orca_safety_space"]) == moved
    if name == "traj_a5_linear_dt01":  # to the time-out: the 31st step of 0.1 s is the first past time_limit = 3
        assert int(z["info"][-1]) == _abi.INFO_TIMEOUT and len(z["info"]) == 31 and not z["done"][:-1].any()


BEGIN, END = "# BEGIN generated by tests/test_params_cpu.py", "# END generated"


def test_write_the_coverage_table():
    """(set x form), the share of humans whose first ORCA velocity a set moves, and the info codes of every run, into
    profiles/param_coverage.txt between the markers; what else the file holds stays.  Written only when it differs."""
    lines = [BEGIN, "# ORCA solver (tests/test_orca_branches_*): humans whose velocity at step 0 differs bitwise from the",
             "# default set's, of the humans that exist", "%-18s %s" % ("case", "changed / humans")]
    for case in ORCA_HUMAN_CASES:
        n, rv, ps = case
        if ps not in ORCA_MOVED_SETS:
            continue
        b = orca_human_batch(n, rv)
        exists = np.arange(n)[None, :] < b.n_humans[:, None]
        a, d = orca_reference(case)["out"][0]["human_action"], orca_reference((n, rv, "default"))["out"][0]["human_action"]
        lines.append("%-18s %d / %d" % (orca_case_id(case), int(((a != d).any(-1) & exists).sum()), int(exists.sum())))
    lines += ["# whole step (tests/test_params_*): E = %d, N = %d, S = %d, %d steps, time_limit %g, auto-reset over %d scenes;"
              % (pc.E, pc.N, pc.S, pc.STEPS, pc.TIME_LIMIT, 2 * pc.E),
              "# steps per info code (0 nothing, 1 danger, 2 goal, 3 obstacle, 4 adult, 5 bicycle, 6 child, 7 time-out)",
              "%-8s %-18s %-10s %s" % ("set", "form", "robot", " ".join("%5d" % c for c in range(8)))]
    for (ps, form, kin), c in _code_counts().items():
        lines.append("%-8s %-18s %-10s %s" % (ps, form, kin, " ".join("%5d" % c.get(code, 0) for code in range(8))))
    lines += ["# the look-ahead runs before every %dth step of the ORCA step runs; ebc_sail_dagger_k: \"all\", %d envs, %d steps;"
              % (pc.LOOKAHEAD_EVERY, pc.DAGGER["E"], pc.DAGGER["K"]),
              "# ebc_step_with_map: dt0.1, unicycle, %d envs, %d steps" % (pc.MAP["E"], pc.MAP["steps"]), END]
    new = "\n".join(lines) + "\n"
    old = open(TABLE).read() if os.path.exists(TABLE) else ""
    if BEGIN in old and END in old:
        text = old[:old.index(BEGIN)] + new + old[old.index(END) + len(END) + 1:]
    else:
        text = old + new
    if text != old:
        with open(TABLE, "w") as f:
            f.write(text)
    assert BEGIN in text and END in text
