"""Shared by tests/test_sail_rollout_cpu.py and tests/test_sail_rollout_gpu.py: the scenes, networks and configurations
of ebc_step_k with EBC_ROBOT_SAIL, and the reference rollout the GPU test compares with — the oracle's step with the g++
host build of the network (sail_cases.host_forward) deciding, K steps, computed once per configuration and process.

Scenes.  Every env has exactly adult_num observation rows (`humans` moving agents and `static` obstacles as pedestrians),
built directly as struct-of-arrays like test_gpu_parity._synthetic_batch: humans in a 4 m box with goals across it, the
robot 6 m from its goal, a few occupied grid cells.  One env per batch (`ARRIVED_ENV`, when the batch has more than one)
starts 0.1 m from its goal, inside its 0.3 m radius: the (0, 0) rule.  No env has another row count: where a NaN action
goes in the step is pinned by no test.

Networks.  The recorded weights of tests/golden/sail_a5.npz for adult_num = 5, sail_cases.random_state_dict(adult_num, 1)
for the other widths.  Both are torch's initialisation (the golden run's torch_seed, no training), so an action is a few
tenths of a metre per second at the most: over K <= 45 steps of 0.25 s a robot moves a few metres at the very most, which
test_sail_rollout_cpu.py checks step by step against BOUND, beside the finiteness of every action."""
import numpy as np

from ebcsim import _abi, scene as ebc_scene
from helpers import load, params_of
from sail_cases import golden, host_forward, random_state_dict

KEYS9 = ("state_rotated", "n_rows", "robot_action_out", "reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated")
BOUND = 4.5  # half of map_size_m = 9: the square the occupancy grid covers
ARRIVED_ENV = 1


def state_dict_of(adult_num):
    return golden("sail_a5")[2] if adult_num == 5 else random_state_dict(adult_num, 1)


def params_for(T=17, kinematics=_abi.HOLONOMIC, time_limit=4.0):
    """The parameters of traj_n10_walls_t17_orcasub (a penalty for every kind of collision); T = 17: rows with the agent
    type as there, T = 13: without."""
    p = params_of(load("traj_n10_walls_t17_orcasub"))
    p.with_agent_type = 1 if T == 17 else 0
    assert _abi.rot_width(p) == T
    p.time_limit = time_limit
    p.robot_kinematics = kinematics
    if kinematics == _abi.UNICYCLE:
        p.rotate_unicycle = 1
        p.rotation_penalty_factor = -0.004
    return p


def full_batch(seed, E, humans, static, arrived=True, walls=True):
    """E scenes of exactly `humans` + `static` rows (N = humans, S = static slots, all in use)."""
    rs = np.random.RandomState(seed)
    N, S = humans, static
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = ebc_scene.SceneBatch(E, N, S, np.full(E, N, np.int32), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                             f(E, N), np.zeros((E, N), np.uint8), np.full(E, S, np.int32), f(E, max(S, 1)), f(E, max(S, 1)),
                             f(E, max(S, 1)), None, f(E, 9))
    for e in range(E):
        b.px[e], b.py[e] = rs.uniform(-4, 4, N), rs.uniform(-4, 4, N)
        b.vx[e], b.vy[e] = rs.uniform(-0.5, 0.5, N), rs.uniform(-0.5, 0.5, N)
        b.gx[e], b.gy[e] = rs.uniform(-4, 4, N), rs.uniform(-4, 4, N)
        b.radius[e], b.v_pref[e] = rs.uniform(0.1, 0.5, N), rs.uniform(0.3, 1.2, N)
        b.type[e] = np.sort(rs.randint(0, 3, N))
        if S:
            b.spx[e], b.spy[e], b.sradius[e] = rs.uniform(-4, 4, S), rs.uniform(-4, 4, S), rs.uniform(0.3, 0.8, S)
        b.robot[e] = [rs.uniform(-1, 1), -3.0, 0, 0, 0.3, 0.0, 3.0, 0.7, np.pi / 2]
    if arrived and E > 1:
        b.robot[ARRIVED_ENV, 5], b.robot[ARRIVED_ENV, 6] = b.robot[ARRIVED_ENV, 0] + 0.1, b.robot[ARRIVED_ENV, 1]
    if walls:
        grid = np.ones((E, 90, 90))
        for e in range(E):
            for _ in range(3):
                x, y = rs.randint(5, 80, 2)
                grid[e, x:x + rs.randint(1, 12), y:y + rs.randint(1, 12)] = 0
        b.grid = np.stack([ebc_scene.pack_grid(g) for g in grid])
    return b


def golden_batch(E=5):
    """E copies of the golden run's scene (5 adults, no static rows) and its parameters."""
    from helpers import batch_from_init
    z = golden("sail_a5")[0]
    return params_of(z), batch_from_init(z, copies=E)


# One-launch = per-step, bit for bit: (id, adult_num, humans, static, T, E, forced envs per workgroup or None, K, flags,
# pool scenes (0 = restarts from the env's own scene), kinematics).  Together: adult_num 2, 5, 10; splits (5, 0) and
# (3, 2); T 13 and 17; E 1, 3, 70; epg 1, 3, 16 against group_envs = 8 (adult_num 5), 4 (10), 8 (2); K 1 and 40; auto-reset
# over an installed pool and none past a terminal step (time_limit 4 s = 16 steps); both kinematics.
AUTO = _abi.FLAG_AUTO_RESET
BITWISE = [
    ("a5-E70-epg3-pool", 5, 5, 0, 17, 70, 3, 40, AUTO, 140, _abi.HOLONOMIC),
    ("a5-E70-epg16-no-reset", 5, 5, 0, 17, 70, 16, 40, 0, 0, _abi.HOLONOMIC),
    ("a5-split32-E70-epg1-T13", 5, 3, 2, 13, 70, 1, 40, AUTO, 0, _abi.HOLONOMIC),
    ("a5-split32-E3-default-epg", 5, 3, 2, 17, 3, None, 40, AUTO, 6, _abi.HOLONOMIC),
    ("a5-E1-K1", 5, 5, 0, 13, 1, None, 1, 0, 0, _abi.HOLONOMIC),
    ("a2-E70-epg16", 2, 2, 0, 17, 70, 16, 40, AUTO, 0, _abi.HOLONOMIC),
    ("a10-E70-epg3-T13", 10, 10, 0, 13, 70, 3, 40, AUTO, 0, _abi.HOLONOMIC),
    ("a10-split-E70-epg16", 10, 8, 2, 17, 70, 16, 1, 0, 0, _abi.HOLONOMIC),
    ("a5-unicycle-E70-epg3", 5, 5, 0, 17, 70, 3, 40, AUTO, 0, _abi.UNICYCLE),
]


def bitwise_setup(case):
    """(params, first batch, pool batch or None, state_dict) of a BITWISE row."""
    tag, A, humans, static, T, E, epg, K, flags, pool, kin = case
    seed = 7000 + 13 * BITWISE.index(case)
    return (params_for(T, kin), full_batch(seed, E, humans, static),
            full_batch(seed + 1, pool, humans, static, arrived=False) if pool else None, state_dict_of(A))


# the configuration of test 2 (K oracle steps with the host build deciding): test_one_launch_equals_k_oracle_steps's
# sizes, flags and parameters for the external robot (E = 70, K = 45, auto-reset, time_limit 4, the T = 17 parameters),
# on scenes that have adult_num rows each
ORACLE_CASE = dict(E=70, K=45, flags=AUTO, humans=5, static=0, seed=31000)

_rollouts = {}


def oracle_rollout(key, params, batch, sd, K, flags=0, pool=None, keys=KEYS9):
    """K oracle steps with host_forward deciding on the oracle's own state -> ({key: [K, ...]}, final get_state(),
    robot positions [K + 1, E, 2]).  Computed once per `key` and left unchanged."""
    if key not in _rollouts:
        from oracle import oracle
        o = oracle.OracleEnv(params, batch.n, batch.N, batch.S)
        o.reset(batch)
        if pool is not None:
            o.set_scene_pool(pool)
        out = {k: [] for k in keys}
        where = [o.get_state()["robot"][:, :2].copy()]
        for k in range(K):
            ob, rot = o.observe()
            n_rows = o.row_counts()
            action = host_forward(sd, o.get_state()["robot"], ob, n_rows, want_feat=False)[0]
            step = o.step(robot_action=action, human_policy=_abi.HUMAN_ORCA, flags=flags)
            step.update(state_rotated=rot, n_rows=n_rows, robot_action_out=action)
            for name in keys:
                out[name].append(step[name])
            where.append(o.get_state()["robot"][:, :2].copy())
        res = ({k: np.stack(v) for k, v in out.items()}, o.get_state(), np.stack(where))
        for a in list(res[0].values()) + list(res[1].values()) + [res[2]]:
            a.setflags(write=False)
        _rollouts[key] = res
    return _rollouts[key]


def oracle_case():
    c = ORACLE_CASE
    params = params_for(17)
    batch = full_batch(c["seed"], c["E"], c["humans"], c["static"])
    return params, batch, state_dict_of(5)


def reference_rollouts():
    """Every configuration a GPU test compares with the reference rollout or runs a closed loop on: (tag, params, batch,
    pool, sd, K, flags).  test_sail_rollout_cpu.py walks them all."""
    params, batch, sd = oracle_case()
    yield "oracle-case", params, batch, None, sd, ORACLE_CASE["K"], ORACLE_CASE["flags"]
    gp, gb = golden_batch(5)
    yield "golden-scene", gp, gb, None, state_dict_of(5), 24, 0
    for case in BITWISE:
        p, b, pool, sd = bitwise_setup(case)
        yield case[0], p, b, pool, sd, case[7], case[8]
