"""ebc_step_k with EBC_FLAG_ONE_LAUNCH (-m gpu): the K steps as ONE kernel launch, a workgroup per group of envs with
the state in LDS between steps (csrc/ebc_rollout.h).  It is held (1) to the oracle with the tolerances of
test_step_k_equals_k_oracle_steps, and (2)-(4) to the per-step form BIT FOR BIT — every output compared as raw bytes,
the state left behind too, and what a per-step continuation computes from it (which reads everything get_state does
not show: float tile, static rows, grid slot, pool cursor).  A difference there is a different operation somewhere,
not a tolerance.  (5) refusals, (6) the trainer."""
import configparser
import json
import os

import numpy as np
import pytest

from ebcsim import _abi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
from helpers import Guarded, load, params_of
from test_gpu_parity import _config_text, _env, _random_batch, _synthetic_batch

pytestmark = pytest.mark.gpu

ONE = _abi.FLAG_ONE_LAUNCH
AUTO = _abi.FLAG_AUTO_RESET
KEYS9 = ("state_rotated", "n_rows", "robot_action_out", "reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eb-cadrl_amd")


def _walls_params():
    z = load("traj_n10_walls_t17_orcasub")
    return params_of(z), _config_text(json.loads(str(z["meta"])))


def _robot_kw(robot, K, E, v_pref, seed=5, kinematics="holonomic"):
    kw = dict(human_policy=_abi.HUMAN_ORCA)
    if robot == "orca":
        kw.update(robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)
    elif robot == "linear":
        kw.update(robot_policy=_abi.ROBOT_LINEAR)
    else:
        space = ebc_actions.build_action_space(v_pref) if kinematics == "holonomic" else \
            ebc_actions.build_action_space(v_pref, "unicycle")
        rs = np.random.RandomState(seed)
        kw.update(robot_policy=_abi.ROBOT_EXTERNAL, robot_action=space[rs.randint(len(space), size=(K, E))])
    return kw


def _bytes_equal(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8), err_msg=tag)


def _state_equal(a, b, sim=False, tag=""):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        _bytes_equal(sa[k], sb[k], tag + " state " + k)
    for x, y, name in zip(a.observe(), b.observe(), ("ob", "obs_rotated")):  # the static rows too
        _bytes_equal(x, y, tag + " observe " + name)
    if sim:
        ra, rb = a.robot_orca_sim_state(), b.robot_orca_sim_state()
        for k in ra:
            _bytes_equal(ra[k], rb[k], tag + " simulator " + k)


def _both(a, b, K, keys, flags, tag, **kw):
    """K steps on `a` per step and on `b` in one launch: every output as raw bytes."""
    oa = a.step_k(K, keys, flags=flags, **kw)
    ob = b.step_k(K, keys, flags=flags | ONE, **kw)
    for k in keys:
        _bytes_equal(oa[k], ob[k], "%s output %s" % (tag, k))
    return oa


def _probe(a, b, flags, sim, tag, steps=10):
    """Both handles continue PER STEP: what they compute shows the state get_state does not (tile, static rows, grid
    slot, pool cursor, the simulators)."""
    _state_equal(a, b, sim, tag)
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA if sim else _abi.ROBOT_LINEAR,
              robot_safety_space=0.15)
    oa = a.step_k(steps, KEYS9, flags=flags, **kw)
    ob = b.step_k(steps, KEYS9, flags=flags, **kw)
    for k in KEYS9:
        _bytes_equal(oa[k], ob[k], "%s continuation %s" % (tag, k))
    _state_equal(a, b, sim, tag + " after continuation")


def _pair(params, E, N, S, setup):
    a, b = _env(params, E, N, S), _env(params, E, N, S)
    for g in (a, b):
        setup(g)
    return a, b


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("robot", ["orca", "linear", "external"])
def test_one_launch_equals_k_oracle_steps(robot):
    """test_step_k_equals_k_oracle_steps with the flag on the GPU side only: its scenes, seeds, sizes and tolerances."""
    from oracle import oracle
    params, text = _walls_params()
    params.time_limit = 4
    E, K = 70, 45
    b, _ = _random_batch(text, [31000 + e for e in range(E)])
    g = _env(params, E, b.N, b.S)
    o = oracle.OracleEnv(params, E, b.N, b.S)
    g.reset(b)
    o.reset(b)
    kw = _robot_kw(robot, K, E, float(b.robot[0, 7]))
    keys = KEYS9 if robot != "external" else tuple(k for k in KEYS9 if k != "robot_action_out")  # as that test
    og = g.step_k(K, keys, flags=AUTO | ONE, **kw)
    oo = o.step_k(K, keys, flags=AUTO, **kw)
    for k in ("done", "info", "n_rows"):
        np.testing.assert_array_equal(og[k], oo[k], err_msg=k)
    for k in ("reward", "dmin", "dist_to_goal", "robot_action_out"):
        if k not in og:
            continue
        both_inf = np.isinf(og[k]) & np.isinf(oo[k])
        np.testing.assert_allclose(np.where(both_inf, 0, og[k]), np.where(both_inf, 0, oo[k]), atol=1e-9, rtol=0, err_msg=k)
    for k in ("state_rotated", "obs_rotated"):
        np.testing.assert_allclose(og[k], oo[k], atol=1e-5, rtol=1e-5, err_msg=k)
    assert int(oo["done"].sum()) > E  # restarts happened inside the launch
    sg, so = g.get_state(), o.get_state()
    for k in sg:
        np.testing.assert_allclose(sg[k], so[k], atol=1e-9, rtol=0, err_msg=k)
    g.synchronize()


def test_one_launch_full_size_vs_oracle():
    """4096 x 10, walls, auto-reset: 32 steps in one launch against 32 oracle steps on the host threads (the scenes
    and seeds of test_full_size_parity_vs_oracle)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from oracle import oracle
    params, text = _walls_params()
    params.time_limit = 6
    E, K = 4096, 32
    b, _ = _random_batch(text, [21000 + e for e in range(E)])
    g = _env(params, E, b.N, b.S)
    o = oracle.OracleEnv(params, E, b.N, b.S)
    g.reset(b)
    o.reset(b)
    g.use_torch_stream()
    keys = ("reward", "done", "info", "obs_rotated")
    outs = g.alloc_step_k_outputs(K, keys)
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR)
    g.step_k_device(outs, K, flags=AUTO | ONE, **kw)
    g.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    oracle.set_threads(bench.host_cores())
    try:
        restarts = 0
        for t in range(K):
            ref = o.step(flags=AUTO, **kw)
            np.testing.assert_array_equal(got["done"][t], ref["done"], err_msg="step %d" % t)
            np.testing.assert_array_equal(got["info"][t], ref["info"], err_msg="step %d" % t)
            np.testing.assert_allclose(got["reward"][t], ref["reward"], atol=1e-9, rtol=0)
            np.testing.assert_allclose(got["obs_rotated"][t], ref["obs_rotated"], atol=1e-5, rtol=1e-5)
            restarts += int(ref["done"].sum())
    finally:
        oracle.set_threads(1)
    assert restarts > E
    sg, so = g.get_state(), o.get_state()
    for k in sg:
        np.testing.assert_allclose(sg[k], so[k], atol=1e-9, rtol=0, err_msg=k)


def _placed_batch(n_humans, n_static, N, S, shift):
    """Scenes placed by hand, free maps.  Robot e starts at (0.1 e, -3) for (0, 3).  Its humans stand 2 m from it on the
    side of its goal, walk towards it at 0.3 m/s and want to pass it; its static obstacles stand 2.5 m behind it.  Every
    radius is its own (and `shift` larger), so a simulator that kept its radii shows which scene built it.  Within the
    0.5 s before the time-out nothing can touch: the gap is 2 m - 0.3 - radius (at most 0.4 + shift), the closing speed
    at most 1 + 0.7 m/s."""
    E = len(n_humans)
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = ebc_scene.SceneBatch(E, N, S, np.asarray(n_humans, np.int32), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                             f(E, N), f(E, N), np.zeros((E, N), np.uint8), np.asarray(n_static, np.int32),
                             f(E, max(S, 1)), f(E, max(S, 1)), f(E, max(S, 1)), None, f(E, 9))
    for e in range(E):
        rx, ry = 0.1 * e, -3.0
        b.robot[e] = [rx, ry, 0, 0, 0.3, 0.0, 3.0, 0.7, np.pi / 2]
        for i in range(n_humans[e]):
            th = 0.5 + 0.9 * i + 0.05 * e
            c, s = np.cos(th), np.sin(th)
            b.px[e, i], b.py[e, i] = rx + 2.0 * c, ry + 2.0 * s
            b.vx[e, i], b.vy[e, i] = -0.3 * c, -0.3 * s
            b.gx[e, i], b.gy[e, i] = rx - 2.0 * c, ry - 2.0 * s
            b.radius[e, i] = 0.2 + 0.05 * i + 0.01 * e + shift
            b.v_pref[e, i] = 1.0
        for j in range(n_static[e]):
            ph = np.pi + 0.9 + 1.3 * j
            b.spx[e, j], b.spy[e, j] = rx + 2.5 * np.cos(ph), ry + 2.5 * np.sin(ph)
            b.sradius[e, j] = 0.3 + 0.1 * j + shift
    return b


def test_one_launch_robot_orca_persistent_simulator_vs_oracle(monkeypatch):
    """The robot on ORCA with the persistent simulator, one launch against the oracle and nothing else: the one-launch
    and the per-step form call the same orca_robot_solve, so their agreement no longer witnesses the simulator rule.
    Five envs, two per workgroup (the last workgroup holds one), scenes placed by hand (_placed_batch: no seed decides
    a row count or a collision).  Every env times out at the third step and restarts
    from its pool scene: one of them onto another row count (the simulator is rebuilt), four onto the same (it keeps
    the radii of the scene that built it); the fourth step is decided from those simulators.  The robot's action bit
    for bit, as test_robot_orca_rollouts_vs_oracle holds the per-step kernel; the rest with the tolerances of
    test_one_launch_equals_k_oracle_steps."""
    from oracle import oracle
    params, _ = _walls_params()
    params.time_limit = 0.5
    E, N, S, K = 5, 3, 2, 4
    first = _placed_batch([3, 2, 3, 1, 2], [1, 2, 0, 2, 1], N, S, 0.0)
    pool = _placed_batch([3, 2, 3, 1, 3], [1, 2, 0, 2, 1], N, S, 0.07)  # env e restarts from pool scene e: the last onto 4 rows, from 3
    rows_first, rows_pool = first.n_humans + first.n_static, pool.n_humans + pool.n_static
    assert int((rows_first != rows_pool).sum()) == 1
    g = _env(params, E, N, S)
    o = oracle.OracleEnv(params, E, N, S)
    for x in (g, o):
        x.reset(first)
        x.set_scene_pool(pool)
        x.robot_orca_sim(True)
    monkeypatch.setenv("EBCSIM_ONE_LAUNCH_EPG", "2")
    kw = _robot_kw("orca", K, E, 0.7)
    og = g.step_k(K, KEYS9, flags=AUTO | ONE, **kw)
    oo = o.step_k(K, KEYS9, flags=AUTO, **kw)
    assert oo["done"][2].all() and not oo["done"][:2].any()  # the restarts lie inside the launch, a step before its end
    for k in ("done", "info", "n_rows"):
        np.testing.assert_array_equal(og[k], oo[k], err_msg=k)
    _bytes_equal(og["robot_action_out"], oo["robot_action_out"], "robot_action_out")
    for k in ("reward", "dmin", "dist_to_goal"):
        both_inf = np.isinf(og[k]) & np.isinf(oo[k])
        np.testing.assert_allclose(np.where(both_inf, 0, og[k]), np.where(both_inf, 0, oo[k]), atol=1e-9, rtol=0, err_msg=k)
    for k in ("state_rotated", "obs_rotated"):
        np.testing.assert_allclose(og[k], oo[k], atol=1e-5, rtol=1e-5, err_msg=k)
    sg, so = g.get_state(), o.get_state()
    for k in sg:
        np.testing.assert_allclose(sg[k], so[k], atol=1e-9, rtol=0, err_msg=k)
    mg, mo = g.robot_orca_sim_state(), o.robot_orca_sim_state()
    np.testing.assert_array_equal(mg["rows"], rows_pool)
    np.testing.assert_array_equal(mg["rows"], mo["rows"])
    _bytes_equal(mg["self"], mo["self"], "simulator self")
    for e in range(E):  # the rows the simulator holds; what lies behind them is never read
        _bytes_equal(mg["radius"][e, :rows_pool[e]], mo["radius"][e, :rows_pool[e]], "simulator radius of env %d" % e)
    kept = np.flatnonzero(rows_first == rows_pool)
    built_from = np.float32(first.radius[kept[0], 0] + 0.01 + 0.15)  # the first scene's human, not the pool scene's
    assert mg["radius"][kept[0], 0] == built_from != np.float32(pool.radius[kept[0], 0] + 0.01 + 0.15)
    g.synchronize()


# ------------------------------------------------------------------ 2. equal to the per-step form, bit for bit
@pytest.mark.parametrize("robot", ["orca", "linear", "external"])
def test_bitwise_three_robots(robot):
    params, text = _walls_params()
    params.time_limit = 4
    E, K = 70, 45
    bt, _ = _random_batch(text, [31000 + e for e in range(E)])
    a, b = _pair(params, E, bt.N, bt.S, lambda g: g.reset(bt))
    kw = _robot_kw(robot, K, E, float(bt.robot[0, 7]))
    out = _both(a, b, K, KEYS9, AUTO, robot, **kw)
    assert int(out["done"].sum()) > E
    _probe(a, b, AUTO, False, robot)


@pytest.mark.parametrize("persistent", [True, False])
def test_bitwise_persistent_simulator_ragged_pool(persistent):
    """Every human and obstacle with its own radius, pool slots with different row counts: with the persistent
    simulator a restart onto a slot with another row count rebuilds it inside the launch, one with the same count
    keeps the radii of the scene that built it."""
    params, _ = _walls_params()
    params.time_limit = 3
    rs = np.random.RandomState(123)
    E, N, S, K = 40, 8, 4, 80
    first = _synthetic_batch(rs, E, N, S, n_lo=1)
    pool = _synthetic_batch(rs, 3 * E, N, S, n_lo=1)
    rows = pool.n_humans + pool.n_static
    assert len(set(rows.tolist())) > 3

    def setup(g):
        g.reset(first)
        g.set_scene_pool(pool)
        g.robot_orca_sim(persistent)
    a, b = _pair(params, E, N, S, setup)
    kw = _robot_kw("orca", K, E, 0.7)
    out = _both(a, b, K, KEYS9, AUTO, "sim %s" % persistent, **kw)
    assert int(out["done"].sum()) > 2 * E
    if persistent:
        sim = b.robot_orca_sim_state()
        assert (sim["rows"] >= 0).all()
    _probe(a, b, AUTO, persistent, "sim %s" % persistent)


def test_bitwise_plain_rows_t13():
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(PKG, "configs", "bench_metric.config"))
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(PKG, "configs", "policy_plain.config"))
    params = ebc_config.params_from_config(cfg, pol)
    params.time_limit = 4
    sc = ebc_scene.SceneConfig.from_config(cfg)
    E, K = 33, 40
    bt = ebc_scene.SceneBatch.from_scenes([ebc_scene.generate_scene(sc, 2000 + e) for e in range(E)])
    a, b = _pair(params, E, bt.N, bt.S, lambda g: g.reset(bt))
    assert a.T == 13
    for robot in ("orca", "linear"):
        _both(a, b, K, KEYS9, AUTO, "T13 " + robot, **_robot_kw(robot, K, E, float(bt.robot[0, 7])))
    _probe(a, b, AUTO, False, "T13")


def test_bitwise_unicycle_external_rotations():
    params, _ = _walls_params()
    params.robot_kinematics = _abi.UNICYCLE
    params.rotate_unicycle = 1
    params.rotation_penalty_factor = -0.004
    params.time_limit = 5
    rs = np.random.RandomState(9)
    E, N, S, K = 70, 5, 0, 40
    bt = _synthetic_batch(rs, E, N, S)
    a, b = _pair(params, E, N, S, lambda g: g.reset(bt))
    kw = _robot_kw("external", K, E, 0.7, kinematics="unicycle")
    out = _both(a, b, K, KEYS9, AUTO, "unicycle", **kw)
    assert out["done"].any()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        _bytes_equal(sa[k], sb[k], "unicycle state " + k)
    out = _both(a, b, 7, KEYS9, 0, "unicycle, no auto-reset", **_robot_kw("external", 7, E, 0.7, seed=6, kinematics="unicycle"))


@pytest.mark.parametrize("visible", [1, 0])
def test_bitwise_robot_visible(visible):
    params, _ = _walls_params()
    params.robot_visible = visible
    params.time_limit = 5
    rs = np.random.RandomState(31)
    E, N, S, K = 70, 6, 2, 40
    bt = _synthetic_batch(rs, E, N, S)
    a, b = _pair(params, E, N, S, lambda g: g.reset(bt))
    for robot in ("linear", "orca"):
        _both(a, b, K, KEYS9, AUTO, "visible %d %s" % (visible, robot), **_robot_kw(robot, K, E, 0.7))
    _probe(a, b, AUTO, False, "visible %d" % visible)


def test_bitwise_installed_pool_smaller_than_the_batch():
    """P = 7 < E, stride 3: envs share pool scenes and walk them with a stride that is not the default."""
    params, _ = _walls_params()
    params.time_limit = 3
    rs = np.random.RandomState(77)
    E, N, S, K = 20, 8, 4, 70
    first = _synthetic_batch(rs, E, N, S, n_lo=2)
    pool = _synthetic_batch(rs, 7, N, S, n_lo=1)

    def setup(g):
        g.reset(first)
        g.set_scene_pool(pool, stride=3)
    a, b = _pair(params, E, N, S, setup)
    out = _both(a, b, K, KEYS9, AUTO, "pool 7", **_robot_kw("linear", K, E, 0.7))
    assert int(out["done"].sum()) > 3 * E
    _probe(a, b, AUTO, False, "pool 7", steps=30)  # through further restarts: the cursors must agree


def _metric_gen():
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(PKG, "configs", "bench_metric.config"))
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(PKG, "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    return params, ebc_scene.gen_struct(sc, "test"), sum(ebc_scene.gen_struct(sc, "test").count), ebc_scene.max_static_rows(sc)


def test_bitwise_device_generated_pool():
    params, gen, N, S = _metric_gen()
    params.time_limit = 4
    E, K = 130, 50

    def setup(g):
        g.generate_reset(gen, 1000)
        g.generate_pool(gen, 100000, 2 * E)
    a, b = _pair(params, E, N, S, setup)
    out = _both(a, b, K, KEYS9, AUTO, "generated pool", **_robot_kw("orca", K, E, 1.0))
    assert int(out["done"].sum()) > E
    _probe(a, b, AUTO, False, "generated pool", steps=25)


@pytest.mark.parametrize("E", [1, 3, 70, 4099])
def test_bitwise_batch_sizes(E):
    """Groups that are not full and a last workgroup that ends past E."""
    params, gen, N, S = _metric_gen()
    params.time_limit = 3
    K = 20

    def setup(g):
        g.generate_reset(gen, 5000)
    a, b = _pair(params, E, N, S, setup)
    for robot in ("orca", "linear"):
        _both(a, b, K, KEYS9, AUTO, "E %d %s" % (E, robot), **_robot_kw(robot, K, E, 1.0))
    _probe(a, b, AUTO, False, "E %d" % E, steps=4)


@pytest.mark.parametrize("N,S", [(7, 3), (1, 0), (24, 6)])
def test_bitwise_ragged_humans_and_no_static_rows(N, S):
    """Envs with fewer humans than max_humans (empty ones too), with zero static rows, a handle without static slots."""
    params, _ = _walls_params()
    params.time_limit = 4
    rs = np.random.RandomState(1000 + N)
    E, K = 70, 40
    bt = _synthetic_batch(rs, E, N, S)
    assert (bt.n_humans < N).any() and (S == 0 or (bt.n_static == 0).any())
    a, b = _pair(params, E, N, S, lambda g: g.reset(bt))
    for robot in ("linear", "orca", "external"):
        _both(a, b, K, KEYS9, AUTO, "ragged %d+%d %s" % (N, S, robot), **_robot_kw(robot, K, E, 0.7))
    _probe(a, b, AUTO, False, "ragged %d+%d" % (N, S))


@pytest.mark.parametrize("K", [1, 200])
def test_bitwise_one_step_and_two_hundred(K):
    params, text = _walls_params()
    params.time_limit = 6
    E = 64
    bt, _ = _random_batch(text, [41000 + e for e in range(E)])
    a, b = _pair(params, E, bt.N, bt.S, lambda g: g.reset(bt))
    _both(a, b, K, KEYS9, AUTO, "K %d" % K, **_robot_kw("orca", K, E, float(bt.robot[0, 7])))
    _probe(a, b, AUTO, False, "K %d" % K, steps=3)


def test_bitwise_without_auto_reset_past_a_terminal_step():
    params, text = _walls_params()
    params.time_limit = 2
    E, K = 64, 30
    bt, _ = _random_batch(text, [42000 + e for e in range(E)])
    a, b = _pair(params, E, bt.N, bt.S, lambda g: g.reset(bt))
    out = _both(a, b, K, KEYS9, 0, "no auto-reset", **_robot_kw("linear", K, E, float(bt.robot[0, 7])))
    assert out["done"][8:].all()  # every env is past its time limit and keeps being stepped
    _probe(a, b, 0, False, "no auto-reset", steps=3)


# ------------------------------------------------------------------ 3. continuation
def test_continuation_between_the_forms():
    """One-launch K = 17, three ebc_step calls and an ebc_lookahead, one-launch K = 9, per-step K = 5, against the same
    sequence all per step."""
    params, text = _walls_params()
    params.time_limit = 3
    E = 70
    bt, _ = _random_batch(text, [43000 + e for e in range(E)])
    a, b = _pair(params, E, bt.N, bt.S, lambda g: g.reset(bt))
    space = ebc_actions.build_action_space(float(bt.robot[0, 7]))
    kw = _robot_kw("orca", 17, E, float(bt.robot[0, 7]))
    _both(a, b, 17, KEYS9, AUTO, "first window", **kw)
    for t in range(3):
        sa = a.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=AUTO)
        sb = b.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=AUTO)
        for k in sa:
            _bytes_equal(sa[k], sb[k], "ebc_step %d %s" % (t, k))
    la = a.lookahead(space, human_policy=_abi.HUMAN_ORCA)
    lb = b.lookahead(space, human_policy=_abi.HUMAN_ORCA)
    for k in la:
        _bytes_equal(la[k], lb[k], "ebc_lookahead " + k)
    _both(a, b, 9, KEYS9, AUTO, "second window", **kw)
    oa = a.step_k(5, KEYS9, flags=AUTO, **kw)
    ob = b.step_k(5, KEYS9, flags=AUTO, **kw)
    for k in KEYS9:
        _bytes_equal(oa[k], ob[k], "per-step tail " + k)
    _state_equal(a, b, False, "end")


# ------------------------------------------------------------------ 4. optional outputs and bounds
def _guarded_outputs(env, K, keys):
    import torch
    shapes = env._STEP_K_SHAPES(env.E, env.R, env.T)
    return {k: Guarded((K,) + shapes[k][0], getattr(torch, shapes[k][1]), tile_rows=1) for k in keys}


@pytest.mark.parametrize("E", [70, 4099])
@pytest.mark.parametrize("keys", [("reward",), ("state_rotated", "obs_rotated"), KEYS9])
def test_optional_outputs_stay_inside_their_buffers(E, keys):
    """Every output buffer between canaries, poisoned inside: all of it written, nothing beside it; equal to the
    per-step form's; the host-location call equals the device-location call."""
    params, gen, N, S = _metric_gen()
    params.time_limit = 3
    K = 12

    def setup(g):
        g.generate_reset(gen, 7000)
        g.use_torch_stream()
    a, b = _pair(params, E, N, S, setup)
    c = _env(params, E, N, S)
    c.generate_reset(gen, 7000)
    kw = _robot_kw("orca", K, E, 1.0)
    ga, gb = _guarded_outputs(a, K, keys), _guarded_outputs(b, K, keys)
    a.step_k_device({k: g.t for k, g in ga.items()}, K, flags=AUTO, **kw)
    b.step_k_device({k: g.t for k, g in gb.items()}, K, flags=AUTO | ONE, **kw)
    a.synchronize()
    b.synchronize()
    host = c.step_k(K, keys, flags=AUTO | ONE, **kw)
    for k in keys:
        want, got = ga[k].check(), gb[k].check()
        _bytes_equal(want, got, "device %s" % k)
        _bytes_equal(host[k], got, "host %s" % k)
    _state_equal(a, b, False, "guarded")


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    import torch
    from ebcsim import _capi
    params, gen, N, S = _metric_gen()
    E, K = 64, 4
    env = _env(params, E, N, S)
    with pytest.raises(_capi.EbcError, match="before ebc_reset") as ei:
        env.step_k(K, ("reward",), flags=ONE, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR)
    assert ei.value.code == _abi.ERR_STATE
    env.generate_reset(gen, 9000)
    env.use_torch_stream()
    env.set_human_actions(np.zeros((E, N, 2)))
    before = env.get_state()
    for policy, name in ((_abi.HUMAN_LINEAR, "EBC_HUMAN_LINEAR"), (_abi.HUMAN_EXTERNAL, "EBC_HUMAN_EXTERNAL")):
        g = _guarded_outputs(env, K, ("reward", "done", "state_rotated"))
        with pytest.raises(_capi.EbcError, match=name) as ei:
            env.step_k_device({k: v.t for k, v in g.items()}, K, flags=AUTO | ONE, human_policy=policy,
                              robot_policy=_abi.ROBOT_LINEAR)
        assert ei.value.code == _abi.ERR_UNSUPPORTED
        env.synchronize()
        for v in g.values():
            v.check(written=False)
        after = env.get_state()
        for k in before:
            _bytes_equal(before[k], after[k], "state after a refused call: " + k)
        # the per-step form takes the same call
        env2 = _env(params, E, N, S)
        env2.generate_reset(gen, 9000)
        env2.set_human_actions(np.zeros((E, N, 2)))
        env2.step_k(K, ("reward",), flags=AUTO, human_policy=policy, robot_policy=_abi.ROBOT_LINEAR)
    with pytest.raises(_capi.EbcError) as ei:
        env.step_k(0, ("reward",), flags=ONE, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR)
    assert ei.value.code == _abi.ERR_INVALID
    with pytest.raises(_capi.EbcError, match="border") as ei:
        env.step_k(K, ("reward",), flags=ONE | _abi.FLAG_BORDER, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR)
    assert ei.value.code == _abi.ERR_UNSUPPORTED
    # a capturing stream
    outs = env.alloc_step_k_outputs(K, ("reward", "done"))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=AUTO | ONE)
    with torch.cuda.stream(side):
        env.use_torch_stream()
        env.step_k_device(outs, K, **kw)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError, match="captured") as ei:
                env.step_k_device(outs, K, **kw)
            assert ei.value.code == _abi.ERR_UNSUPPORTED
        finally:
            graph.capture_end()
        env.step_k_device(outs, K, **kw)
        side.synchronize()
    env.synchronize()  # returns OK: a one-launch call has no mailbox to time out on


# ------------------------------------------------------------------ 6. the trainer
def test_collect_il_one_launch_fills_the_same_memory():
    import torch
    from ebcsim.train import DeviceReplay, collect_il
    params, _ = _walls_params()
    params.time_limit = 4
    rs = np.random.RandomState(321)
    E, N, S, steps = 48, 8, 4, 60
    first = _synthetic_batch(rs, E, N, S, n_lo=1)
    pool = _synthetic_batch(rs, 2 * E, N, S, n_lo=1)
    mems, counts = [], []
    for one in (False, True):
        env = _env(params, E, N, S)
        env.reset(first)
        env.set_scene_pool(pool)
        env.use_torch_stream()
        mem = DeviceReplay(steps * E, env.R, env.T, torch.device("cuda", 0))
        counts.append(collect_il(env, mem, steps, 0.9, 0.15, persistent_sim=True, one_launch=one))
        mems.append(mem)
    assert counts[0] == counts[1] and counts[0][0] > 0 and counts[0][1] > E
    n = counts[0][0]
    assert torch.equal(mems[0].states[:n], mems[1].states[:n])
    assert torch.equal(mems[0].values[:n], mems[1].values[:n])
    assert torch.equal(mems[0].n_valid[:n], mems[1].n_valid[:n])
