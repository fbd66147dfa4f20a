"""Shared by tests/test_sail_dagger_cpu.py and tests/test_sail_dagger_gpu.py: the configurations of ebc_sail_dagger_k (the
SAIL network drives, the ORCA robot labels every state, a mask says whose action a step executes), their masks, and the
same rollout walked on the oracle — observe, row_counts, robot_orca, the g++ host build of the network
(sail_cases.host_forward), the mask, step — computed once per case and process.

Scenes and networks are those of tests/sail_rollout_cases.py (every env has exactly adult_num rows; untrained weights, so
the learner's actions are a few tenths of a metre per second; the expert heads for a goal 6 m away at 0.7 m/s at the
most).  time_limit is 4 s = 16 steps, so a K = 20 window with auto-reset crosses restarts."""
import numpy as np

from ebcsim import _abi
from sail_cases import host_forward
from sail_rollout_cases import full_batch, params_for, state_dict_of

AUTO = _abi.FLAG_AUTO_RESET
SAFETY = 0.15  # the expert's safety_space (rl/train.py:127-129 sets the demonstrator's)

# (id, adult_num, humans, static, T, E, K, flags, pool scenes (0 = restarts from the env's own scene), persistent
# simulator of the expert, mask: "random" (p = 0.5), "ones", or None (NULL: the learner always acts)).
# GS = the lanes of a robot group, the smallest of 2 3 4 5 6 7 8 9 10 12 16 21 32 that holds adult_num rows.
CASES = [
    ("a5-E70-K20-pool-random", 5, 5, 0, 17, 70, 20, AUTO, 140, False, "random"),   # restarts from an installed pool
    ("a5-split32-E3-K20-sim-random", 5, 3, 2, 13, 3, 20, AUTO, 0, True, "random"),  # static rows, persistent simulator
    ("a2-E70-K6-null", 2, 2, 0, 17, 70, 6, 0, 0, False, None),                      # GS 2: 32 envs per wave, E no multiple
    ("a10-split82-E70-K6-ones", 10, 8, 2, 17, 70, 6, 0, 0, False, "ones"),          # GS 10: 4 idle lanes per wave
    ("a11-E7-K3", 11, 11, 0, 17, 7, 3, 0, 0, False, "random"),                      # GS 12 with a rowless lane
    ("a17-E4-K3", 17, 17, 0, 17, 4, 3, 0, 0, False, "random"),                      # GS 21: 3 groups and one idle lane
    ("a32-E3-K3", 32, 32, 0, 17, 3, 3, 0, 0, False, "random"),                      # GS 32
    ("a5-E1-K1", 5, 5, 0, 17, 1, 1, 0, 0, False, "ones"),                           # the smallest call
]


def seed_of(case):
    return 9100 + 17 * CASES.index(case)


def mask_of(case):
    """take_expert [K, E] uint8, or None."""
    tag, A, humans, static, T, E, K, flags, pool, sim, mask = case
    if mask is None:
        return None
    if mask == "ones":
        return np.ones((K, E), np.uint8)
    return (np.random.RandomState(seed_of(case) + 5).uniform(size=(K, E)) < 0.5).astype(np.uint8)


def setup(case):
    """(params, first batch, pool batch or None, state_dict, mask) of a CASES row."""
    tag, A, humans, static, T, E, K, flags, pool, sim, mask = case
    seed = seed_of(case)
    return (params_for(T), full_batch(seed, E, humans, static),
            full_batch(seed + 1, pool, humans, static, arrived=False) if pool else None, state_dict_of(A), mask_of(case))


OUT = ("robot", "ob", "n_rows", "learner_action", "expert_action", "robot_action_out", "reward", "done", "info")
_walks = {}


def select(mask_k, expert, learner):
    """The entry's item 4 on the host: whole float64 words chosen."""
    return learner.copy() if mask_k is None else np.where(mask_k.astype(bool)[:, None], expert, learner)


def oracle_walk(case):
    """The rollout of `case` on the oracle -> ({name: [K, ...]} for OUT, final get_state(), robot positions
    [K + 1, E, 2]).  Computed once per case and left unchanged."""
    tag = case[0]
    if tag not in _walks:
        from oracle import oracle
        _, A, humans, static, T, E, K, flags, pool_n, sim, _ = case
        params, batch, pool, sd, mask = setup(case)
        o = oracle.OracleEnv(params, batch.n, batch.N, batch.S)
        o.reset(batch)
        if pool is not None:
            o.set_scene_pool(pool)
        o.robot_orca_sim(bool(sim))
        out = {k: [] for k in OUT}
        where = [o.get_state()["robot"][:, :2].copy()]
        for k in range(K):
            rec = dict(robot=o.get_state()["robot"].copy(), ob=o.observe()[0], n_rows=o.row_counts())
            rec["expert_action"] = o.robot_orca(SAFETY)
            rec["learner_action"] = host_forward(sd, rec["robot"], rec["ob"], rec["n_rows"], want_feat=False)[0]
            rec["robot_action_out"] = select(None if mask is None else mask[k], rec["expert_action"], rec["learner_action"])
            step = o.step(robot_action=rec["robot_action_out"], human_policy=_abi.HUMAN_ORCA, flags=flags)
            rec.update(reward=step["reward"], done=step["done"], info=step["info"])
            for name in OUT:
                out[name].append(np.array(rec[name]))
            where.append(o.get_state()["robot"][:, :2].copy())
        res = ({k: np.stack(v) for k, v in out.items()}, o.get_state(), np.stack(where))
        for a in list(res[0].values()) + list(res[1].values()) + [res[2]]:
            a.setflags(write=False)
        _walks[tag] = res
    return _walks[tag]


# the schedule test (tests/test_sail_dagger_gpu.py, test 6): 64 envs of 5 adults whose robot starts 2 m from its goal, so
# that the demonstrator ends episodes in ReachGoal inside a 24-step window (2 m at 0.7 m/s is 12 steps; time_limit 6 s)
SCHEDULE = dict(E=64, demo_steps=24, dagger_steps=24, rounds=2, epochs=2, seed=9900, time_limit=6.0)


def schedule_setup():
    c = SCHEDULE
    params = params_for(17, time_limit=c["time_limit"])
    batch = full_batch(c["seed"], c["E"], 5, 0, arrived=False)
    batch.robot[:, 1], batch.robot[:, 6] = -1.0, 1.0
    return params, batch, state_dict_of(5)
