"""The crowd rules — mixed, mixed_20, one_static (scene_generator.py:523-589) — on the device (-m gpu): scene_gen_kernel
against the g++ build of the same source (every bit, cos / sin included) and against the reference's own scenes (the bar
of tests/test_crowd_rules_cpu.py); the generated scenes through reset, the auto-reset pool and 120 steps against the
oracle, on the 21-lane ORCA groups (mixed_20) and on the 5-lane ones with row counts that change at every restart
(mixed); the reference-run mixed_20 episode through the C ABI; a SARL decision on a ragged generated batch; refusals."""
import configparser
import copy
import os

import numpy as np
import pytest

from ebcsim import _abi, _capi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
from crowd_rules_cases import CAPACITY, compare, golden_sets
from helpers import GOLDEN, batch_from_init, check_trajectory, load, params_of
from test_gpu_parity import _compare_step
from test_scene_gen import host_gen  # noqa: F401  (the fixture: the g++ build of the generator)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sets():
    return golden_sets()


def _params(text, policy_config=None):
    cfg = configparser.RawConfigParser()
    cfg.read_string(text)
    if policy_config is None:
        return ebc_config.params_from_config(cfg)
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", policy_config))
    return ebc_config.params_from_config(cfg, pol)


def test_kernel_equals_host_build_and_goldens(host_gen, sets):  # noqa: F811
    from ebcsim.batched import BatchedEnv
    differ = total = 0
    for gs in sets:  # mixed, mixed_20, one_static, and mixed_20 with random attributes, bicycles, children and a map
        want = gs.batch(1, 2)
        assert want.N == CAPACITY[gs.rule] + gs.cfg.bicycle_num + gs.cfg.children_num + 1
        gen = ebc_scene.gen_struct(gs.cfg, "test")
        env = BatchedEnv(_params(gs.text), 8, want.N, want.S)
        seeds = np.asarray(gs.seeds, np.uint32)
        got = env.generate_scenes(gen, seeds, len(seeds))
        rc, host = host_gen(gen, seeds, want.N, want.S, env.G)
        assert rc == 0
        compare(got, host, gs.tag + ": device vs host build", exact=True)
        assert gs.seeds == list(range(gs.seeds[0], gs.seeds[0] + len(seeds)))
        compare(env.generate_scenes(gen, gs.seeds[0], len(seeds)), host, gs.tag + ": seed0 form", exact=True)
        d, t = compare(got, want, gs.tag + ": device vs reference")
        differ, total = differ + d, total + t
        env.close()
    assert total > 2000 and differ <= total // 100, (differ, total)


@pytest.mark.parametrize("rule,N", [("mixed_20", 20), ("mixed", 6)])
def test_generate_reset_and_pool_against_oracle(sets, rule, N):
    """The shape of tests/test_scene_gen.py::test_generate_reset_and_pool_against_oracle on generated crowds: 32 envs, a
    pool of 64 scenes, 120 auto-reset steps with ORCA humans and the linear robot, every output against the oracle.
    mixed_20 fills its 20 slots (21-lane groups); mixed has one slot to spare and 1 to 5 adults per scene, so an env's
    row count changes from one restart to the next (5-lane groups)."""
    from ebcsim.batched import BatchedEnv
    from oracle import oracle
    gs = next(s for s in sets if s.rule == rule and not s.randomized)
    gen = ebc_scene.gen_struct(gs.cfg, "test")
    params = _params(gs.text)
    params.time_limit = 5
    E, S = 32, 0
    g = BatchedEnv(params, E, N, S)
    o = oracle.OracleEnv(params, E, N, S)
    pool_seeds = np.arange(50000, 50000 + 2 * E, dtype=np.uint32)
    first = g.generate_scenes(gen, 1000, E)
    pool = g.generate_scenes(gen, pool_seeds, 2 * E)
    if rule == "mixed":
        assert len(set(first.n_humans.tolist())) > 2 and len(set(pool.n_humans.tolist())) > 2
    else:
        assert (first.n_humans == 20).all() and (pool.n_humans == 20).all()
    o.reset(first)
    o.set_scene_pool(pool)
    g.generate_reset(gen, 1000)
    g.generate_pool(gen, pool_seeds, 2 * E)
    assert g.ragged
    sg, so = g.get_state(), o.get_state()
    for k in sg:
        np.testing.assert_array_equal(sg[k], so[k], err_msg=k)
    restarts, changed, rows = 0, False, g.row_counts().copy()
    for t in range(120):
        og = g.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET)
        oo = o.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET)
        _compare_step(og, oo, "%s: generated pool step %d" % (rule, t))
        restarts += int(og["done"].sum())
        if og["done"].any():
            now = g.row_counts().copy()
            changed = changed or bool((now != rows).any())
            rows = now
    assert restarts >= E  # time_limit 5 = 20 steps: every env restarts several times
    if rule == "mixed":
        assert changed  # some env went on with a scene of another size
    np.testing.assert_array_equal(g.row_counts(), o.row_counts())
    g.close()


def test_reference_episode_through_the_c_abi():
    """tests/golden/traj_mix20_orcasub.npz as tests/test_gpu_parity.py replays its `_orcasub` fixtures."""
    from ebcsim.batched import BatchedEnv
    z = load("traj_mix20_orcasub")
    b = batch_from_init(z, copies=3)
    assert b.N == 20
    env = BatchedEnv(params_of(z), 3, b.N, b.S)
    env.reset(b)
    check_trajectory(env, z, atol=1e-9)
    env.close()


def test_decisions_on_a_ragged_generated_batch(sets):
    """mixed_20 with random attributes, bicycles, children and a map: the rows a SARL decision sees are the generated
    scenes' humans + static rows, and the matrix-core blocks choose what the float32 torch path chooses, in every env."""
    import torch
    from ebcsim.batched import BatchedEnv
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    gs = sets[-1]
    assert gs.rule == "mixed_20" and gs.randomized
    gen = ebc_scene.gen_struct(gs.cfg, "test")
    params = _params(gs.text, "policy_agent_type.config")
    E = 32
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(gs.cfg))
    scenes = env.generate_scenes(gen, 3000, E)
    env.generate_reset(gen, 3000)
    env.use_torch_stream()
    assert env.ragged
    space = ebc_actions.build_action_space(gs.cfg.robot.v_pref)
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device="cuda:0")
    policy = DeviceSarlPolicy(net, space, 0.9)
    actions, values = policy.decide(env)
    torch.cuda.synchronize()
    actions = actions.clone()
    assert net.native_forwards > 0
    rows = scenes.n_humans + scenes.n_static
    assert len(set(rows.tolist())) > 1 and rows.max() <= env.R
    np.testing.assert_array_equal(policy.n_valid.cpu().numpy(), rows)
    plain = SarlValueNet.from_stacks(net.mlp1, net.mlp2, net.attention, net.mlp3, net.with_global_state, net.self_state_dim,
                                     "cuda:0", native=False)
    want, _ = DeviceSarlPolicy(plain, space, 0.9).decide(env)
    torch.cuda.synchronize()
    assert plain.native_forwards == 0
    np.testing.assert_array_equal(actions.cpu().numpy(), want.cpu().numpy())
    env.close()


def test_refusals(sets):
    from ebcsim.batched import BatchedEnv
    gs = next(s for s in sets if s.rule == "mixed_20" and not s.randomized)
    gen = ebc_scene.gen_struct(gs.cfg, "test")
    params = _params(gs.text)
    with pytest.raises(_capi.EbcError, match="max_humans"):
        BatchedEnv(params, 4, 19, 0).generate_reset(gen, 1)
    low = copy.deepcopy(gen)
    low.count[0] = 0  # not read under a crowd rule: the capacity still counts
    with pytest.raises(_capi.EbcError, match="max_humans"):
        BatchedEnv(params, 4, 19, 0).generate_reset(low, 1)
    BatchedEnv(params, 4, 20, 0).generate_reset(low, 1)
    for code, name in ((_abi.RULE_MIXED, "mixed"), (_abi.RULE_MIXED_20, "mixed_20"), (_abi.RULE_ONE_STATIC, "one_static")):
        for t in (1, 2):
            bad = copy.deepcopy(gen)
            bad.rule[t] = code
            with pytest.raises(_capi.EbcError, match="the %s rule" % name):
                BatchedEnv(params, 4, 24, 0).generate_reset(bad, 1)
    # a code that is no rule, on a type with no humans (a caller that left rule[0] unset): nothing is placed for it, as
    # before the crowd rules; with humans to place it is refused
    for code in (6, 7, -1):
        unset = copy.deepcopy(gen)
        unset.rule[0], unset.count[0] = code, 0
        env = BatchedEnv(params, 4, 2, 0)
        assert not env.generate_scenes(unset, np.array([3050, 3038, 3000, 3001], np.uint32), 4).n_humans.any()
        env.generate_reset(unset, 3050)
        assert not env.row_counts().any()
        unset.count[0] = 1
        with pytest.raises(_capi.EbcError, match="EbcSceneGen.rule"):
            env.generate_reset(unset, 3050)
        env.close()
