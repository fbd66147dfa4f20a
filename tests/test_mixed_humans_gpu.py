"""Humans on a policy per entity type on the device (-m gpu): EBC_HUMAN_BY_TYPE with ebc_set_human_policies through
ebc_step (the mixed instantiation of the fused step), ebc_lookahead, and ebc_step_k in its per-step and one-launch forms.

Bars, from the project's own tests: what is downstream of exact inputs is compared as raw bytes (the ORCA humans of a
mixed step against an EBC_HUMAN_ORCA step from the same state, a mixed step against the EBC_HUMAN_EXTERNAL step given its
velocities, the one-launch form against the per-step form); where a linear human's double-precision atan2 / sin / cos is
computed by two different kernels or by the checker the bar is 1e-9 (tests/test_rotated_rows_gpu.py,
tests/test_state_buffers_gpu.py hold EBC_HUMAN_LINEAR there), 1e-5 for float32 rotated rows, masks and codes exact.

Shapes: N = 1 (the robot the only other), 3, 6, 10, 17, and 33 with S = 32 (ORCA groups of 2 to 32 lanes; R = 65 > 64,
where the ROWS role takes two passes); E = 1 and 37 (partial ENV and STATE waves); all eight tables at N = 6; types grouped
and interleaved, ragged batches; env 0 of every batch has no human of a linear type and env 1 only such humans."""
import numpy as np
import pytest

from ebcsim import _abi, _capi, actions as ebc_actions, scene as ebc_scene
from helpers import batch_from_init, check_trajectory, load, params_of
from mixed_humans import (ADULTS_LINEAR, ALL_TABLES, BIKES_LINEAR, BY_TYPE, LINEAR, ORCA, AsMixed, MixedOracle, same_bytes,
                          table_of)

pytestmark = pytest.mark.gpu

AUTO, ONE = _abi.FLAG_AUTO_RESET, _abi.FLAG_ONE_LAUNCH
NAME = "traj_mixed_a3b3c2"
STEP_KEYS = ("reward", "done", "info", "dmin", "dist_to_goal", "robot_action_out", "human_action", "ob", "obs_rotated")
_made = []


def make_env(params, E, N, S):
    from ebcsim.batched import BatchedEnv
    _made.append(BatchedEnv(params, E, N, S))
    return _made[-1]


@pytest.fixture(autouse=True)
def fault_word_never_raised():
    del _made[:]
    yield
    for env in _made:
        env.synchronize()  # EBC_OK, or EbcError: no mailbox wait of any launch of the test gave up


def params_for(visible=0, typed=False, kinematics="holonomic", time_limit=None):
    p = params_of(load(NAME))
    p.robot_visible = int(visible)
    p.with_agent_type = int(typed)
    if kinematics != "holonomic":
        p.robot_kinematics, p.rotate_unicycle = _abi.UNICYCLE, 1
    if time_limit is not None:
        p.time_limit = time_limit
    return p


def scenes(seed, E, N, S, table, interleaved=False, ragged=False):
    """Random scenes as SoA.  Env 0 has no human of a type `table` puts on linear, env 1 (when there is one) only such
    humans, where the table has both kinds; the others draw all three types, grouped by type or interleaved."""
    rs = np.random.RandomState(seed)
    n = rs.randint(1, N + 1, size=E).astype(np.int32) if ragged else np.full(E, N, np.int32)
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = ebc_scene.SceneBatch(E, N, S, n, f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                             np.zeros((E, N), np.uint8), rs.randint(0, S + 1, size=E).astype(np.int32) if S else np.zeros(E, np.int32),
                             f(E, max(S, 1)), f(E, max(S, 1)), f(E, max(S, 1)), None, f(E, 9))
    on_orca = [t for t in range(3) if table[t] == ORCA]
    on_linear = [t for t in range(3) if table[t] == LINEAR]
    for e in range(E):
        k = n[e]
        b.px[e, :k], b.py[e, :k] = rs.uniform(-4, 4, k), rs.uniform(-4, 4, k)
        b.vx[e, :k], b.vy[e, :k] = rs.uniform(-0.5, 0.5, k), rs.uniform(-0.5, 0.5, k)
        b.gx[e, :k], b.gy[e, :k] = rs.uniform(-4, 4, k), rs.uniform(-4, 4, k)
        b.radius[e, :k], b.v_pref[e, :k] = rs.uniform(0.1, 0.5, k), rs.uniform(0.3, 1.2, k)
        pool = on_orca if (e == 0 and on_orca) else on_linear if (e == 1 and on_linear) else [0, 1, 2]
        types = np.array(pool)[rs.randint(0, len(pool), k)]
        b.type[e, :k] = types if interleaved else np.sort(types)
        m = b.n_static[e]
        b.spx[e, :m], b.spy[e, :m], b.sradius[e, :m] = rs.uniform(-4, 4, m), rs.uniform(-4, 4, m), rs.uniform(0.3, 0.8, m)
        b.robot[e] = [rs.uniform(-1, 1), -3.0, 0, 0, 0.3, rs.uniform(-1, 1), 3.0, 0.7, np.pi / 2]
    return b


def robot_actions(seed, shape, kinematics="holonomic"):
    space = ebc_actions.build_action_space(0.7) if kinematics == "holonomic" else ebc_actions.build_action_space(0.7, "unicycle")
    return space[np.random.RandomState(seed).randint(len(space), size=shape)]


def on_linear(batch_types, table):
    return np.array(tuple(table) + (ORCA,))[np.minimum(batch_types, 3)] == LINEAR


def assert_bytes(a, b, keys, tag):
    for k in keys:
        assert same_bytes(a[k], b[k]), "%s: %s differs, max %g" % (tag, k, float(np.nanmax(np.abs(
            np.where(np.isinf(a[k].astype(np.float64)) & np.isinf(b[k].astype(np.float64)), 0, a[k].astype(np.float64) - b[k].astype(np.float64))))))


def assert_close(a, b, keys, tag, atol=1e-9):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype == np.uint8 or x.dtype.kind in "iu":
            np.testing.assert_array_equal(x, y, err_msg="%s %s" % (tag, k))
        elif x.dtype == np.float32:
            np.testing.assert_allclose(x, y, atol=1e-5, rtol=1e-5, err_msg="%s %s" % (tag, k))
        else:
            both_inf = np.isinf(x) & np.isinf(y) & (np.sign(x) == np.sign(y))
            np.testing.assert_allclose(np.where(both_inf, 0, x), np.where(both_inf, 0, y), atol=atol, rtol=0, err_msg="%s %s" % (tag, k))


# (N, S, E, table, interleaved, ragged, robot_visible, 17-wide rows, kinematics)
SHAPES = [
    (1, 0, 37, BIKES_LINEAR, False, False, 1, False, "holonomic"),
    (3, 2, 1, ADULTS_LINEAR, True, False, 0, True, "holonomic"),
    (6, 3, 37, BIKES_LINEAR, True, True, 1, True, "holonomic"),
    (10, 8, 37, ADULTS_LINEAR, False, True, 0, False, "holonomic"),
    (17, 0, 37, BIKES_LINEAR, True, False, 1, False, "unicycle"),
    (33, 32, 37, ADULTS_LINEAR, False, True, 0, True, "holonomic"),  # 32 others: the robot is not one of them
]
SHAPE_IDS = ["N%d-S%d-E%d" % s[:3] for s in SHAPES]


# ------------------------------------------------------------------ 1. uniform tables are the plain policies
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_uniform_tables_equal_the_plain_steps(shape):
    N, S, E, _, interleaved, ragged, visible, typed, kin = shape
    E = 37
    params = params_for(visible, typed, kin, time_limit=2)
    b = scenes(100 + N, E, N, S, BIKES_LINEAR, interleaved, ragged)
    acts = robot_actions(N, (12, E), kin)
    for code in (ORCA, LINEAR):
        mixed, plain = make_env(params, E, N, S), make_env(params, E, N, S)
        mixed.set_human_policies(code, code, code)
        assert mixed.human_policies == (code, code, code) and plain.human_policies == (ORCA, ORCA, ORCA)
        for env in (mixed, plain):
            env.reset(b)
        restarts = 0
        for t in range(12):
            om = mixed.step(robot_action=acts[t], human_policy=BY_TYPE, flags=AUTO)
            op = plain.step(robot_action=acts[t], human_policy=code, flags=AUTO)
            tag = "table of three %s, step %d" % ("ORCA" if code == ORCA else "LINEAR", t)
            if code == ORCA:
                assert_bytes(om, op, STEP_KEYS, tag)
                assert_bytes(mixed.get_state(), plain.get_state(), plain.get_state().keys(), tag + " state")
            else:
                assert_close(om, op, STEP_KEYS, tag)
                assert_close(mixed.get_state(), plain.get_state(), plain.get_state().keys(), tag + " state")
            restarts += int(op["done"].sum())
        assert restarts > 0  # time_limit 2 s: every env restarts inside the 12 steps


# ------------------------------------------------------------------ 2. exact, without the checker
def exact_chain(N, S, E, table, interleaved, ragged, visible, typed, kin, k=8):
    params = params_for(visible, typed, kin)
    b = scenes(200 + 7 * N + sum(table), E, N, S, table, interleaved, ragged)
    acts = robot_actions(N + 1, (k + 1, E), kin)
    envs = [make_env(params, E, N, S) for _ in range(4)]
    for env in envs:
        env.reset(b)
        env.set_human_policies(*table)
        for t in range(k):
            env.step(robot_action=acts[t], human_policy=BY_TYPE)
    mixed, orca, linear, external = envs
    types = mixed.get_state()["type"]
    live = np.arange(N)[None, :] < mixed.get_state()["n_humans"][:, None]
    lin = on_linear(types, table) & live
    om = mixed.step(robot_action=acts[k], human_policy=BY_TYPE)
    oo = orca.step(robot_action=acts[k], human_policy=ORCA)
    ol = linear.step(robot_action=acts[k], human_policy=LINEAR)
    tag = "N %d table %s" % (N, (table,))
    assert same_bytes(om["human_action"][live & ~lin], oo["human_action"][live & ~lin]), tag + ": the humans on ORCA"
    assert same_bytes(om["human_action"][lin], ol["human_action"][lin]), tag + ": the humans on linear"
    assert not om["human_action"][~live].any()
    if lin.any() and (live & ~lin).any():  # a mixed step is neither of the two
        assert not same_bytes(om["human_action"], oo["human_action"]) and not same_bytes(om["human_action"], ol["human_action"])
    external.set_human_actions(om["human_action"])
    oe = external.step(robot_action=acts[k], human_policy=_abi.HUMAN_EXTERNAL)
    assert_bytes(om, oe, STEP_KEYS, tag + ": against EBC_HUMAN_EXTERNAL given the mixed velocities")
    assert_bytes(mixed.get_state(), external.get_state(), mixed.get_state().keys(), tag + " state")
    # what get_state does not show (the float tile): both continue with an ORCA step
    a, c = mixed.step(robot_action=acts[0], human_policy=ORCA), external.step(robot_action=acts[0], human_policy=ORCA)
    assert_bytes(a, c, STEP_KEYS, tag + " continuation")
    return lin, live


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_step_is_exact_per_type_and_equals_the_external_step(shape):
    lin, live = exact_chain(*shape)
    N, E = shape[0], shape[2]
    if E > 1 and N > 1:
        assert not lin[0].any() and (lin[1] == live[1]).all()  # env 0: nobody on linear; env 1: everybody


@pytest.mark.parametrize("table", ALL_TABLES, ids=["".join("L" if c == LINEAR else "O" for c in t) for t in ALL_TABLES])
def test_every_table_at_six_humans(table):
    exact_chain(6, 3, 37, table, True, True, 1, False, "holonomic", k=5)


# ------------------------------------------------------------------ 3. one device step from distinct visited states
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[5]], ids=[SHAPE_IDS[2], SHAPE_IDS[3], SHAPE_IDS[5]])
def test_one_step_from_visited_states_against_the_checker(shape):
    N, S, _, table, interleaved, ragged, visible, typed, kin = shape
    params = params_for(visible, typed, kin)
    K = 12
    start = scenes(300 + N, 4, N, S, table, interleaved, False)
    walker = MixedOracle(params, 4, N, S)
    walker.reset(start)
    walker.set_human_policies(*table)
    acts = robot_actions(N + 2, (K, 4), kin)
    # every visited state of envs 2 and 3 (all three types) becomes one env of a scene of 2 K
    b = scenes(300 + N, 2 * K, N, S, table, interleaved, False)
    for t in range(K):
        st = walker.get_state()
        for e in (2, 3):
            q = 2 * t + e - 2
            for key in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type"):
                getattr(b, key)[q] = st[key][e]
            b.n_humans[q], b.robot[q] = st["n_humans"][e], st["robot"][e]
            b.n_static[q] = start.n_static[e]
            b.spx[q], b.spy[q], b.sradius[q] = start.spx[e], start.spy[e], start.sradius[e]
        walker.step(robot_action=acts[t], human_policy=BY_TYPE)
    E = 2 * K
    dev, chk = make_env(params, E, N, S), MixedOracle(params, E, N, S)
    for env in (dev, chk):
        env.reset(b)
        env.set_human_policies(*table)
    act = robot_actions(N + 3, (E,), kin)
    od = dev.step(robot_action=act, human_policy=BY_TYPE)
    oc = chk.step(robot_action=act, human_policy=BY_TYPE)
    assert_close(od, oc, STEP_KEYS, "one step from %d visited states" % E)
    sd, sc = dev.get_state(), chk.get_state()
    assert_close(sd, sc, sc.keys(), "state")
    lin = on_linear(b.type, table)
    assert lin.any() and (~lin).any()


# ------------------------------------------------------------------ 4. look-ahead, then the cached step
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=[SHAPE_IDS[1], SHAPE_IDS[2], SHAPE_IDS[4]])
def test_mixed_lookahead_then_cached_step(shape):
    N, S, E, table, interleaved, ragged, visible, typed, kin = shape
    params = params_for(visible, typed, kin)
    b = scenes(400 + N, E, N, S, table, interleaved, ragged)
    space = ebc_actions.build_action_space(0.7) if kin == "holonomic" else ebc_actions.build_action_space(0.7, "unicycle")
    space = space[::5]
    looked, stepped, chk = make_env(params, E, N, S), make_env(params, E, N, S), MixedOracle(params, E, N, S)
    for env in (looked, stepped, chk):
        env.reset(b)
        env.set_human_policies(*table)
    for t in range(4):
        la = looked.lookahead(space, human_policy=BY_TYPE)
        lc = chk.lookahead(space, human_policy=BY_TYPE)
        assert_close(la, lc, ("done", "info", "reward", "dmin", "next_ob", "rows_rotated"), "sweep %d" % t)
        act = space[np.random.RandomState(t).randint(len(space), size=E)]
        oc = looked.step(robot_action=act, human_policy=_abi.HUMAN_CACHED)
        om = stepped.step(robot_action=act, human_policy=BY_TYPE)
        assert_close(om, oc, STEP_KEYS, "cached step %d" % t)
        lin = on_linear(b.type, table)
        assert same_bytes(om["human_action"][~lin], oc["human_action"][~lin]), "the ORCA humans of the cache"
        assert_close(looked.get_state(), stepped.get_state(), stepped.get_state().keys(), "state %d" % t)
        chk.step(robot_action=act, human_policy=BY_TYPE)


# ------------------------------------------------------------------ 5. ebc_step_k
K_KEYS = ("state_rotated", "n_rows", "robot_action_out", "reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated")


def robot_kw(robot, K, E):
    if robot == "orca":
        return dict(robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)
    if robot == "linear":
        return dict(robot_policy=_abi.ROBOT_LINEAR)
    return dict(robot_policy=_abi.ROBOT_EXTERNAL, robot_action=robot_actions(55, (K, E)))


@pytest.mark.parametrize("robot", ["external", "linear", "orca"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_step_k_per_step_and_one_launch(shape, robot):
    N, S, E, table, interleaved, ragged, visible, typed, _ = shape
    params = params_for(visible, typed, time_limit=2)
    K = 14
    b = scenes(500 + N, E, N, S, table, interleaved, ragged)
    pool = scenes(600 + N, 5, N, S, table, not interleaved, ragged)
    calls, per_step, one = (make_env(params, E, N, S) for _ in range(3))
    for env in (calls, per_step, one):
        env.reset(b)
        env.set_scene_pool(pool, stride=3)
        env.set_human_policies(*table)
    kw = robot_kw(robot, K, E)
    keys = K_KEYS if robot != "external" else tuple(k for k in K_KEYS if k != "robot_action_out")
    op = per_step.step_k(K, keys, flags=AUTO, human_policy=BY_TYPE, **kw)
    oo = one.step_k(K, keys, flags=AUTO | ONE, human_policy=BY_TYPE, **kw)
    assert_bytes(op, oo, keys, "one launch against the per-step form, robot %s" % robot)
    assert_bytes(per_step.get_state(), one.get_state(), one.get_state().keys(), "state")
    assert int(op["done"].sum()) >= E  # restarts inside the window
    # K ebc_step calls, given the actions the window took
    took = kw["robot_action"] if robot == "external" else op["robot_action_out"]
    for t in range(K):
        o = calls.step(robot_action=took[t], human_policy=BY_TYPE, flags=AUTO)
        for k in ("reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated"):
            assert same_bytes(o[k], op[k][t]), "K ebc_step calls: step %d %s" % (t, k)
    assert_bytes(calls.get_state(), per_step.get_state(), calls.get_state().keys(), "state after K calls")
    # both forms continue from what they left behind (float tile, cursor): a further window of either form
    a = per_step.step_k(6, keys, flags=AUTO | ONE, human_policy=BY_TYPE, **robot_kw(robot, 6, E))
    c = one.step_k(6, keys, flags=AUTO, human_policy=BY_TYPE, **robot_kw(robot, 6, E))
    assert_bytes(a, c, keys, "continuation")


def test_all_linear_table_rolls_linear_humans_out_in_one_launch():
    N, S, E, K = 6, 3, 37, 14
    params = params_for(1, False, time_limit=2)
    b = scenes(700, E, N, S, BIKES_LINEAR, True, True)
    one, plain = make_env(params, E, N, S), make_env(params, E, N, S)
    for env in (one, plain):
        env.reset(b)
    one.set_human_policies(LINEAR, LINEAR, LINEAR)
    oo = one.step_k(K, K_KEYS, flags=AUTO | ONE, human_policy=BY_TYPE, robot_policy=_abi.ROBOT_LINEAR)
    op = plain.step_k(K, K_KEYS, flags=AUTO, human_policy=LINEAR, robot_policy=_abi.ROBOT_LINEAR)
    assert_close(oo, op, K_KEYS, "all-linear table in one launch against K EBC_HUMAN_LINEAR steps")
    assert_close(one.get_state(), plain.get_state(), plain.get_state().keys(), "state")
    assert int(op["done"].sum()) >= E
    with pytest.raises(_capi.EbcError, match="EBC_HUMAN_LINEAR") as ei:  # the plain code stays refused under the flag
        plain.step_k(K, ("reward",), flags=AUTO | ONE, human_policy=LINEAR, robot_policy=_abi.ROBOT_LINEAR)
    assert ei.value.code == _abi.ERR_UNSUPPORTED


# ------------------------------------------------------------------ 6. the reference's mixed run on the device
def test_golden_trajectory_on_the_device():
    z = load(NAME)
    b = batch_from_init(z, copies=3)
    env = make_env(params_of(z), 3, b.N, b.S)
    env.reset(b)
    check_trajectory(AsMixed(env, table_of(z)), z, atol=1e-9)


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    import torch
    N, S, E = 6, 3, 37
    params = params_for(1, False)
    env = make_env(params, E, N, S)
    for bad, name in (((ORCA, _abi.HUMAN_EXTERNAL, ORCA), "EBC_BICYCLE"), ((BY_TYPE, ORCA, ORCA), "EBC_ADULT"),
                      ((ORCA, ORCA, _abi.HUMAN_CACHED), "EBC_CHILD"), ((ORCA, ORCA, 7), "EBC_CHILD")):
        with pytest.raises(_capi.EbcError, match=name) as ei:
            env.set_human_policies(*bad)
        assert ei.value.code == _abi.ERR_INVALID
    assert env.human_policies == (ORCA, ORCA, ORCA)  # a refused table changes nothing
    env.set_human_policies(*BIKES_LINEAR)
    for call in (lambda: env.step(human_policy=BY_TYPE, robot_policy=_abi.ROBOT_LINEAR),
                 lambda: env.lookahead(np.zeros((1, 2)), human_policy=BY_TYPE),
                 lambda: env.step_k(2, ("reward",), human_policy=BY_TYPE, robot_policy=_abi.ROBOT_LINEAR),
                 lambda: env.step_k(2, ("reward",), human_policy=BY_TYPE, robot_policy=_abi.ROBOT_LINEAR, flags=ONE)):
        with pytest.raises(_capi.EbcError, match="before ebc_reset") as ei:
            call()
        assert ei.value.code == _abi.ERR_STATE
    env.reset(scenes(800, E, N, S, BIKES_LINEAR))
    with pytest.raises(_capi.EbcError, match="human_policy") as ei:
        env.step(human_policy=5, robot_policy=_abi.ROBOT_LINEAR)
    assert ei.value.code == _abi.ERR_INVALID
    outs = env.alloc_step_outputs(("reward", "done"))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    kw = dict(human_policy=BY_TYPE, robot_policy=_abi.ROBOT_LINEAR)
    with torch.cuda.stream(side):
        env.use_torch_stream()
        env.step_device(outs, **kw)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError, match="captured") as ei:
                env.step_device(outs, **kw)
            assert ei.value.code == _abi.ERR_UNSUPPORTED
        finally:
            graph.capture_end()
        env.step_device(outs, **kw)
        side.synchronize()
