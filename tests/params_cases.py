"""Shared by tests/test_params_cpu.py and tests/test_params_gpu.py: the whole step with EbcParams.time_step, orca_time_horizon
and orca_safety_space off the values every golden has (0.25, 5, 0) — the parameter sets of helpers.ORCA_PARAM_SETS, the
batch, the supplied robot actions, and what the oracle computes for every form a GPU test holds a kernel to, computed once
per process and left unchanged.

The batch is in the style of test_gpu_parity._synthetic_batch: E = 37 envs, up to N = 6 humans (ragged, empty envs) and up
to S = 9 static rows (more static rows than humans), a few occupied grid cells.  Four envs in nine are built so that a
given info code comes up at once (robot inside its goal radius, a block of occupied cells on the robot, an adult on the
robot, an adult just outside it); the pool scenes are built the same way, so restarts meet them again.

time_limit = 1.3 s is a multiple of neither 0.1 nor 0.5, and 0.1 is inexact: the clock is a sum of inexact steps and the
step that starts with it at or past the limit must be the oracle's: the 14th at 0.1, the 4th at 0.5 (and the 7th at the
default 0.25).  With auto-reset over a pool of 2 E scenes every env restarts inside the 30 steps at every set."""
import numpy as np

from ebcsim import _abi, actions as ebc_actions, scene as ebc_scene
from helpers import ORCA_PARAM_SETS, orca_case_params

AUTO, ONE = _abi.FLAG_AUTO_RESET, _abi.FLAG_ONE_LAUNCH
E, N, S, STEPS, TIME_LIMIT = 37, 6, 9, 30, 1.3
SETS = ("dt0.1", "dt0.5", "all")
KINEMATICS = ("holonomic", "unicycle")
LOOKAHEAD_EVERY = 5
ROBOT_SAFETY = 0.15
FIELDS = ("time_step", "orca_time_horizon", "orca_safety_space")
KEYS9 = ("state_rotated", "n_rows", "robot_action_out", "reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated")
# ebc_step_k, per step and as one launch: (robot, kinematics, persistent simulator of the ORCA robot)
STEP_K_FORMS = [("external", "holonomic", False), ("external", "unicycle", False), ("linear", "holonomic", False),
                ("orca", "holonomic", True), ("orca", "holonomic", False)]


def case_params(ps, kin="holonomic", **fields):
    """The parameters of a set (helpers.orca_case_params: its five ORCA and step fields on the T = 17 walls parameters),
    the robot visible under "all" (the humans' safety space then goes onto the robot's radius too), time_limit 1.3;
    `fields` puts single fields back, for the runs the CPU test compares with."""
    p = orca_case_params(int(ps == "all"), ps)
    p.time_limit = TIME_LIMIT
    if kin == "unicycle":
        p.robot_kinematics, p.rotate_unicycle, p.rotation_penalty_factor = _abi.UNICYCLE, 1, -0.004
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def default_fields(ps, names=FIELDS):
    """{field: its default} for the fields of `names` that set `ps` moves."""
    d = dict(zip(FIELDS, ORCA_PARAM_SETS["default"][2:]))
    moved = dict(zip(FIELDS, ORCA_PARAM_SETS[ps][2:]))
    return {k: d[k] for k in names if moved[k] != d[k]}


def step_batch(seed, n, n_lo=0):
    rs = np.random.RandomState(seed)
    f = lambda *s: np.zeros(s)  # noqa: E731
    nh = rs.randint(n_lo, N + 1, size=n).astype(np.int32)
    b = ebc_scene.SceneBatch(n, N, S, nh, f(n, N), f(n, N), f(n, N), f(n, N), f(n, N), f(n, N), f(n, N), f(n, N),
                             np.zeros((n, N), np.uint8), rs.randint(0, S + 1, size=n).astype(np.int32), f(n, S), f(n, S),
                             f(n, S), None, f(n, 9))
    grid = np.ones((n, 90, 90))
    for e in range(n):
        kind = e % 9
        if kind in (2, 3):
            b.n_humans[e] = max(b.n_humans[e], 1)
        k, m = b.n_humans[e], b.n_static[e]
        b.px[e, :k], b.py[e, :k] = rs.uniform(-4, 4, k), rs.uniform(-4, 4, k)
        b.vx[e, :k], b.vy[e, :k] = rs.uniform(-0.5, 0.5, k), rs.uniform(-0.5, 0.5, k)
        b.gx[e, :k], b.gy[e, :k] = rs.uniform(-4, 4, k), rs.uniform(-4, 4, k)
        b.radius[e, :k], b.v_pref[e, :k] = rs.uniform(0.1, 0.5, k), rs.uniform(0.3, 1.2, k)
        b.type[e, :k] = np.sort(rs.randint(0, 3, k))
        b.spx[e, :m], b.spy[e, :m], b.sradius[e, :m] = rs.uniform(-4, 4, m), rs.uniform(-4, 4, m), rs.uniform(0.3, 0.8, m)
        rx = rs.uniform(-1, 1)
        b.robot[e] = [rx, -3.0, 0, 0, 0.3, 0.0, 3.0, 0.7, np.pi / 2]
        for _ in range(3):
            x, y = rs.randint(5, 80, 2)
            grid[e, x:x + rs.randint(1, 12), y:y + rs.randint(1, 12)] = 0
        if kind == 0:  # inside the goal's radius
            b.robot[e, 5], b.robot[e, 6] = rx + 0.1, -3.0
        elif kind == 1:  # occupied cells on and around the robot
            cx, cy = int((rx + 4.5) / 0.1), int((-3.0 + 4.5) / 0.1)
            grid[e, cx - 4:cx + 5, cy - 4:cy + 5] = 0
        elif kind == 2:  # an adult on the robot
            b.px[e, 0], b.py[e, 0], b.type[e, 0] = rx + 0.2, -3.0, 0
        elif kind == 3:  # an adult standing 0.05 m from the robot's hull, the other humans out of the way
            b.px[e, 0], b.py[e, 0], b.vx[e, 0], b.vy[e, 0], b.radius[e, 0], b.type[e, 0] = rx, -3.65, 0, 0, 0.3, 0
            b.gx[e, 0], b.gy[e, 0] = rx, -3.65
            b.py[e, 1:k] = np.abs(b.py[e, 1:k])
    b.grid = np.stack([ebc_scene.pack_grid(g) for g in grid])
    return b


_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def batches():
    """(first batch, pool of 2 E scenes)"""
    return _once("batches", lambda: (step_batch(8100, E), step_batch(8101, 2 * E, n_lo=1)))


def action_space(kin):
    return ebc_actions.build_action_space(0.7) if kin == "holonomic" else ebc_actions.build_action_space(0.7, "unicycle")


def robot_actions(kin):
    """[STEPS, E, 2] from the robot's action space."""
    space = action_space(kin)
    return _once(("act", kin), lambda: space[np.random.RandomState(8102).randint(len(space), size=(STEPS, E))])


def _freeze(x):
    if isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    elif isinstance(x, np.ndarray):
        x.setflags(write=False)
    return x


def start(env, sim=None):
    first, pool = batches()
    env.reset(first)
    env.set_scene_pool(pool)
    if sim is not None:
        env.robot_orca_sim(sim)
    return env


def oracle_env(params, sim=None):
    from oracle import oracle
    return start(oracle.OracleEnv(params, E, N, S), sim)


def step_walk(params, kin, humans, steps=STEPS, lookahead=False):
    """STEPS oracle steps with the supplied robot actions, auto-reset over the pool: dict(out=[per step], state=[after
    each], la={step: look-ahead over the action space before it}).  humans: _abi.HUMAN_LINEAR or HUMAN_ORCA."""
    o = oracle_env(params)
    act = robot_actions(kin)
    ref = dict(out=[], state=[], la={})
    for t in range(steps):
        if lookahead and t % LOOKAHEAD_EVERY == 0:
            ref["la"][t] = o.lookahead(action_space(kin), human_policy=humans)
        ref["out"].append(o.step(robot_action=act[t], human_policy=humans, flags=AUTO))
        ref["state"].append(o.get_state())
    return ref


def step_reference(ps, kin, humans):
    return _once(("step", ps, kin, humans),
                 lambda: _freeze(step_walk(case_params(ps, kin), kin, humans, lookahead=humans == _abi.HUMAN_ORCA)))


def step_k_kw(robot, kin):
    kw = dict(human_policy=_abi.HUMAN_ORCA)
    if robot == "orca":
        kw.update(robot_policy=_abi.ROBOT_ORCA, robot_safety_space=ROBOT_SAFETY)
    elif robot == "linear":
        kw.update(robot_policy=_abi.ROBOT_LINEAR)
    else:
        kw.update(robot_policy=_abi.ROBOT_EXTERNAL, robot_action=robot_actions(kin))
    return kw


def step_k_keys(robot):
    return tuple(k for k in KEYS9 if k != "robot_action_out" or robot != "external")


def step_k_walk(params, robot, kin, sim):
    o = oracle_env(params, sim)
    out = o.step_k(STEPS, step_k_keys(robot), flags=AUTO, **step_k_kw(robot, kin))
    return dict(out=out, state=o.get_state(), sim=o.robot_orca_sim_state() if sim else None)


def step_k_reference(ps, form):
    robot, kin, sim = form
    return _once(("step_k", ps) + form, lambda: _freeze(step_k_walk(case_params(ps, kin), robot, kin, sim)))


def form_id(form):
    return "%s-%s%s" % (form[0], form[1], "-sim" if form[2] else "")


# ---- ebc_sail_dagger_k under "all": 37 envs of 5 adults, 8 steps, a pool, time_limit 0.5 s (the fifth step of 0.1 s is
# past it: every env restarts inside the window), a random mask
DAGGER = dict(E=37, A=5, K=8, seed=8200, time_limit=0.5, safety=ROBOT_SAFETY)


def dagger_setup():
    """(params, first batch, pool, state_dict, mask [K, E])"""
    from sail_rollout_cases import full_batch, params_for, state_dict_of
    c = DAGGER
    p = params_for(17, time_limit=c["time_limit"])
    (p.orca_max_neighbors, p.orca_neighbor_dist, p.time_step, p.orca_time_horizon,
     p.orca_safety_space) = ORCA_PARAM_SETS["all"]
    mask = (np.random.RandomState(c["seed"] + 5).uniform(size=(c["K"], c["E"])) < 0.5).astype(np.uint8)
    return (p, full_batch(c["seed"], c["E"], c["A"], 0), full_batch(c["seed"] + 1, 2 * c["E"], c["A"], 0, arrived=False),
            state_dict_of(c["A"]), mask)


# ---- ebc_step_with_map: a unicycle robot under dt0.1 on generated wall scenes
MAP = dict(E=37, seed=8300, steps=4, dim=48, max_range=3.0)


def map_setup():
    """(params, scene batch with its polygons, robot actions [steps, E, 2] (v, rotation))"""
    import configparser
    import os
    from ebcsim import config as ebc_config
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eb-cadrl_amd", "configs")
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(pkg, "bench_metric.config"))
    pol.read(os.path.join(pkg, "policy_agent_type.config"))
    p = ebc_config.params_from_config(cfg, pol)
    p.robot_kinematics, p.rotate_unicycle, p.time_step = _abi.UNICYCLE, 1, 0.1
    sc = ebc_scene.SceneConfig.from_config(cfg)
    c = MAP
    b = ebc_scene.SceneBatch.from_scenes([ebc_scene.generate_scene(sc, c["seed"] + e) for e in range(c["E"])])
    rs = np.random.RandomState(c["seed"])
    act = np.stack([rs.uniform(0, 4.0, (c["steps"], c["E"])), rs.uniform(-np.pi, np.pi, (c["steps"], c["E"]))], -1)
    return p, b, act


# ---- the Python layer that reads time_step
def sarl_setup(time_step, copies=5):
    """The sarl_a5_baseline scene, `copies` times, at a time step: (params, batch, action space, gamma, weights path)"""
    import json
    import os
    from helpers import GOLDEN, batch_from_init, load, params_of
    z = load("sarl_a5_baseline")
    meta = json.loads(str(z["meta"]))
    p = params_of(z)
    p.time_step = time_step
    return p, batch_from_init(z, copies=copies), z["action_space"], meta["gamma"], os.path.join(GOLDEN, "weights", meta["weights"])


IL = dict(E=16, steps=20, gamma=0.9, safety=ROBOT_SAFETY, seed=8400, time_limit=1.3)
EVAL = dict(E=8, gamma=0.9, safety=ROBOT_SAFETY, seed=8510, time_limit=6.0)  # goals, collisions, time-outs, danger steps


def near_goal_batch(seed, n, time_step, time_limit):
    """5 adults, no static rows, the robot 2 m from its goal (sail_dagger_cases.schedule_setup's scenes): the ORCA robot
    ends episodes in ReachGoal inside a few steps.  -> (params at `time_step`, batch)"""
    from sail_rollout_cases import full_batch, params_for
    p = params_for(17, time_limit=time_limit)
    p.time_step = time_step
    b = full_batch(seed, n, 5, 0, arrived=False)
    b.robot[:, 1], b.robot[:, 6] = -1.0, 1.0
    return p, b


def il_walk():
    """collect_il's window on the oracle at dt0.1: the ORCA robot (persistent simulator) for IL["steps"] steps with
    auto-reset -> rewards, done, info [steps, E]."""
    def make():
        from oracle import oracle
        c = IL
        p, b = near_goal_batch(c["seed"], c["E"], 0.1, c["time_limit"])
        o = oracle.OracleEnv(p, b.n, b.N, b.S)
        o.reset(b)
        o.robot_orca_sim(True)
        return _freeze(o.step_k(c["steps"], ("state_rotated", "reward", "done", "info"), flags=AUTO, human_policy=_abi.HUMAN_ORCA,
                                robot_policy=_abi.ROBOT_ORCA, robot_safety_space=c["safety"]))
    return _once("il", make)


def eval_walk():
    """evaluate()'s episodes on the oracle at dt0.5, the robot on ORCA: (params, per-step reward, done, info, dmin)."""
    def make():
        from oracle import oracle
        c = EVAL
        p, b = near_goal_batch(c["seed"], c["E"], 0.5, c["time_limit"])
        o = oracle.OracleEnv(p, b.n, b.N, b.S)
        o.reset(b)
        steps = int(round(p.time_limit / p.time_step) + 2)
        return p, _freeze(o.step_k(steps, ("reward", "done", "info", "dmin"), flags=0, human_policy=_abi.HUMAN_ORCA,
                                   robot_policy=_abi.ROBOT_ORCA, robot_safety_space=c["safety"]))
    return _once("eval", make)


def eval_tally(p, out):
    """avg_nav_time and the danger frequency of Explorer.run_k_episodes (explorer.py:33-131), plainly: every env up to
    and including its first terminal step."""
    done, info = out["done"].astype(bool), out["info"]
    steps, n = done.shape
    assert done.any(0).all()
    first = done.argmax(0)
    final = info[first, np.arange(n)]
    end_time = np.where(final == _abi.INFO_TIMEOUT, p.time_limit, (first + 1) * p.time_step)
    alive = np.arange(steps)[:, None] <= first[None, :]
    danger = int(((info == _abi.INFO_DANGER) & alive).sum())
    ok = final == _abi.INFO_REACH_GOAL
    return dict(avg_nav_time=float(end_time[ok].mean()) if ok.any() else p.time_limit,
                danger=danger / (end_time.sum() / p.time_step), success=int(ok.sum()), danger_steps=danger, final=final)
