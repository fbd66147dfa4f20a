"""ebc_step_k with EBC_ROBOT_SAIL (-m gpu): the SAIL network as the robot policy of a K-step call.  (1) the per-step
form is DeviceSailPolicy.decide + step_device in bytes; (2) it is K oracle steps with the g++ host build deciding, within
the tolerances of test_one_launch_equals_k_oracle_steps, its actions the host build's bytes; (3) the one-launch form (the
network inside the rollout kernel) is the per-step form bit for bit, outputs and the state left behind; (4) continuation
between the forms; (5) optional outputs between canaries; (6) refusals; (7) the evaluation in windows.  Scenes, networks
and the reference rollout: tests/sail_rollout_cases.py (test_sail_rollout_cpu.py checks its inputs)."""
import configparser

import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi, scene as ebc_scene
from helpers import Guarded, params_of
from sail_cases import golden, host_forward, random_state_dict, same_bytes
from sail_rollout_cases import (AUTO, BITWISE, KEYS9, ORACLE_CASE, bitwise_setup, full_batch, golden_batch, oracle_case,
                                oracle_rollout, params_for, state_dict_of)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE = _abi.FLAG_ONE_LAUNCH
SAIL = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_SAIL)
_nets = {}


def net_of(adult_num):
    from ebcsim.sail import SailNet
    if adult_num not in _nets:
        _nets[adult_num] = SailNet(state_dict_of(adult_num), device=DEV)
    return _nets[adult_num]


def make_env(params, batch, net, pool=None):
    from ebcsim.batched import BatchedEnv
    env = BatchedEnv(params, batch.n, batch.N, batch.S)
    env.reset(batch)
    if pool is not None:
        env.set_scene_pool(pool)
    env.attach_sail(net)
    return env


def _bytes_equal(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8), err_msg=tag)


def _state_equal(a, b, tag):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        _bytes_equal(sa[k], sb[k], tag + " state " + k)
    for x, y, name in zip(a.observe(), b.observe(), ("ob", "obs_rotated")):  # the static rows too
        _bytes_equal(x, y, tag + " observe " + name)


# ------------------------------------------------------------------ 1. the per-step form is the composition, in bytes
def test_per_step_form_equals_decide_and_step_device_bytes():
    from ebcsim.sail import DeviceSailPolicy
    E, K = 5, 12
    params, batch = golden_batch(E)
    net = net_of(5)
    a, b = make_env(params, batch, net), make_env(params, batch, net)
    for env in (a, b):
        env.use_torch_stream()
    before = net.native_forwards
    outs = a.alloc_step_k_outputs(K, KEYS9)
    a.step_k_device(outs, K, **SAIL)
    a.synchronize()
    assert net.native_forwards == before  # the C path does not go through SailNet
    pol = DeviceSailPolicy(net)
    step_keys = ("reward", "done", "info", "dmin", "dist_to_goal", "robot_action_out", "obs_rotated")
    so = b.alloc_step_outputs(step_keys)
    for k in range(K):
        want = dict(state_rotated=b.observe()[1], n_rows=b.row_counts())
        actions, _ = pol.decide(b)
        b.step_device(so, robot_action=actions, human_policy=_abi.HUMAN_ORCA)
        b.synchronize()
        want.update({name: so[name].cpu().numpy() for name in step_keys})
        _bytes_equal(actions.cpu().numpy(), want["robot_action_out"], "the step's own copy of the action, step %d" % k)
        for name in KEYS9:
            _bytes_equal(outs[name][k].cpu().numpy(), want[name], "step %d %s" % (k, name))
    assert net.native_forwards == before + K
    assert bool(torch.isfinite(outs["robot_action_out"]).all()) and bool((outs["n_rows"] == 5).all())
    _state_equal(a, b, "after %d steps" % K)


# ------------------------------------------------------------------ 2. K oracle steps with the host build deciding
def test_per_step_form_equals_k_oracle_steps_with_the_host_build_deciding():
    """E = 70, K = 45, auto-reset, time_limit 4 and the tolerances of test_one_launch_equals_k_oracle_steps (external
    robot): masks and row counts equal, float64 outputs and the final state within 1e-9, rotated rows within 1e-5.  The
    actions are the host build's BYTES on the inputs the device itself had at each step (a twin env advanced a step per
    call shows them), and the twin's 45 one-step calls give the bytes of the one 45-step call."""
    c = ORACLE_CASE
    params, batch, sd = oracle_case()
    E, K = c["E"], c["K"]
    want, want_state, _ = oracle_rollout("oracle-case", params, batch, sd, K, c["flags"])
    net = net_of(5)
    g, twin = make_env(params, batch, net), make_env(params, batch, net)
    og = g.step_k(K, KEYS9, flags=c["flags"], **SAIL)
    for k in range(K):
        robot, ob, n_rows = twin.get_state()["robot"], twin.observe()[0], twin.row_counts()
        one = twin.step_k(1, KEYS9, flags=c["flags"], **SAIL)
        host = host_forward(sd, robot, ob, n_rows, want_feat=False)[0]
        assert same_bytes(one["robot_action_out"][0], host), "step %d: the kernel's action is not the host build's" % k
        for name in KEYS9:
            _bytes_equal(og[name][k], one[name][0], "step %d %s: one call of K against K calls of one" % (k, name))
    for k in ("done", "info", "n_rows"):
        np.testing.assert_array_equal(og[k], want[k], err_msg=k)
    for k in ("reward", "dmin", "dist_to_goal"):
        both_inf = np.isinf(og[k]) & np.isinf(want[k])
        np.testing.assert_allclose(np.where(both_inf, 0, og[k]), np.where(both_inf, 0, want[k]), atol=1e-9, rtol=0, err_msg=k)
    for k in ("state_rotated", "obs_rotated"):
        np.testing.assert_allclose(og[k], want[k], atol=1e-5, rtol=1e-5, err_msg=k)
    assert int(want["done"].sum()) > E  # restarts happened inside the call
    sg = g.get_state()
    for k in sg:
        np.testing.assert_allclose(sg[k], want_state[k], atol=1e-9, rtol=0, err_msg=k)
    print("max |action - oracle rollout's action| %.3g" % float(np.abs(og["robot_action_out"] - want["robot_action_out"]).max()))


# ------------------------------------------------------------------ 3. one-launch = per-step, bit for bit
@pytest.mark.parametrize("case", BITWISE, ids=lambda c: c[0])
def test_one_launch_equals_per_step_bitwise(case, monkeypatch):
    tag, A, humans, static, T, E, epg, K, flags, pool_n, kin = case
    params, batch, pool, sd = bitwise_setup(case)
    net = net_of(A)
    a, b = make_env(params, batch, net, pool), make_env(params, batch, net, pool)
    assert a.T == T and a.R == A
    if epg is not None:
        monkeypatch.setenv("EBCSIM_ONE_LAUNCH_EPG", str(epg))
    oa = a.step_k(K, KEYS9, flags=flags, **SAIL)
    ob = b.step_k(K, KEYS9, flags=flags | ONE, **SAIL)
    for k in KEYS9:
        _bytes_equal(oa[k], ob[k], "%s output %s" % (tag, k))
    assert np.isfinite(oa["robot_action_out"]).all() and (oa["n_rows"] == A).all()
    if E > 1:
        assert (oa["robot_action_out"][0, 1] == 0).all() and oa["robot_action_out"][0, 0].any()  # the (0, 0) rule, and not elsewhere
    if flags and K == 40:
        assert int(oa["done"].sum()) > E
    if not flags and K == 40:
        assert oa["done"][17:].all()  # past the terminal step, without a restart
    _state_equal(a, b, tag)
    # both continue PER STEP: what they compute shows the state get_state does not (tile, static rows, grid slot, cursor)
    ca, cb = a.step_k(5, KEYS9, flags=flags, **SAIL), b.step_k(5, KEYS9, flags=flags, **SAIL)
    for k in KEYS9:
        _bytes_equal(ca[k], cb[k], "%s continuation %s" % (tag, k))
    # the rollout of the host build on the oracle, where the configuration is one of the reference rollouts: the masks
    want = oracle_rollout(tag, params, batch, sd, K, flags, pool)[0]
    np.testing.assert_array_equal(oa["n_rows"], want["n_rows"])


# ------------------------------------------------------------------ 4. continuation
def test_continuation_between_the_forms():
    """K per step then K in one launch, K in one launch then K per step, 2 K per step and 2 K in one launch: the same."""
    K = 9
    params = params_for(17)
    batch, pool = full_batch(8100, 70, 3, 2), full_batch(8101, 70, 3, 2, arrived=False)
    net = net_of(5)
    runs = {}
    for name, plan in (("per-step", [(2 * K, 0)]), ("one-launch", [(2 * K, ONE)]), ("per-step, one-launch", [(K, 0), (K, ONE)]),
                       ("one-launch, per-step", [(K, ONE), (K, 0)])):
        env = make_env(params, batch, net, pool)
        parts = [env.step_k(k, KEYS9, flags=AUTO | extra, **SAIL) for k, extra in plan]
        runs[name] = ({k: np.concatenate([p[k] for p in parts]) for k in KEYS9}, env)
    ref, ref_env = runs["per-step"]
    for name, (out, env) in runs.items():
        for k in KEYS9:
            _bytes_equal(out[k], ref[k], "%s %s" % (name, k))
        _state_equal(env, ref_env, name)


# ------------------------------------------------------------------ 5. optional outputs and bounds
def _guarded_outputs(env, K, keys):
    shapes = env._STEP_K_SHAPES(env.E, env.R, env.T)
    return {k: Guarded((K,) + shapes[k][0], getattr(torch, shapes[k][1]), tile_rows=1) for k in keys}


@pytest.mark.parametrize("keys", [("reward",), ("robot_action_out",), ("state_rotated", "obs_rotated"), ("n_rows", "dmin", "done"), KEYS9])
def test_optional_outputs_stay_inside_their_buffers(keys):
    """Every output buffer between canaries, poisoned inside: all of it written, nothing beside it, in both forms (without
    robot_action_out the action lives in the handle's scratch); the host-location call equals the device-location call."""
    E, K = 70, 12
    params = params_for(17)
    batch = full_batch(8200, E, 5, 0)
    net = net_of(5)
    a, b, c = (make_env(params, batch, net) for _ in range(3))
    for env in (a, b):
        env.use_torch_stream()
    ga, gb = _guarded_outputs(a, K, keys), _guarded_outputs(b, K, keys)
    a.step_k_device({k: g.t for k, g in ga.items()}, K, flags=AUTO, **SAIL)
    b.step_k_device({k: g.t for k, g in gb.items()}, K, flags=AUTO | ONE, **SAIL)
    a.synchronize()
    b.synchronize()
    host = c.step_k(K, keys, flags=AUTO | ONE, **SAIL)
    for k in keys:
        want, got = ga[k].check(), gb[k].check()
        _bytes_equal(want, got, "device %s" % k)
        _bytes_equal(host[k], got, "host %s" % k)
    _state_equal(a, b, "guarded")
    _state_equal(c, b, "guarded, host location")


# ------------------------------------------------------------------ 6. refusals
def _refused(env, K, code, match, flags=0, **kw):
    """A refused device-location call: the code, the message, guarded outputs untouched, state bytes untouched."""
    before = env.get_state()
    g = _guarded_outputs(env, K, ("reward", "robot_action_out", "state_rotated"))
    call = dict(SAIL)
    call.update(kw)
    with pytest.raises(_capi.EbcError, match=match) as ei:
        env.step_k_device({k: v.t for k, v in g.items()}, K, flags=flags, **call)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    env.synchronize()
    for v in g.values():
        v.check(written=False)
    after = env.get_state()
    for k in before:
        _bytes_equal(before[k], after[k], "state after a refused call: " + k)


def test_refusals():
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailNet
    E, K = 8, 4
    params = params_for(17)
    batch = full_batch(8300, E, 5, 0)
    net = net_of(5)
    env = BatchedEnv(params, E, batch.N, batch.S)
    env.attach_sail(net)
    with pytest.raises(_capi.EbcError, match="before ebc_reset") as ei:
        env.step_k(K, ("reward",), **SAIL)
    assert ei.value.code == _abi.ERR_STATE
    env.reset(batch)
    env.use_torch_stream()
    # no network attached (never, and after a detach), both forms
    bare = BatchedEnv(params, E, batch.N, batch.S)
    bare.reset(batch)
    bare.use_torch_stream()
    for flags in (0, ONE):
        _refused(bare, K, _abi.ERR_STATE, "no network attached", flags=flags)
    bare.attach_sail(net)
    bare.step_k(K, ("reward",), **SAIL)
    bare.attach_sail(None)
    _refused(bare, K, _abi.ERR_STATE, "no network attached")
    # EBC_ROBOT_SAIL belongs to ebc_step_k
    with pytest.raises(_capi.EbcError, match="robot_policy") as ei:
        env.step(robot_policy=_abi.ROBOT_SAIL)
    assert ei.value.code == _abi.ERR_INVALID
    # fewer rows than adult_num: the attach is refused and leaves the env without a network; DeviceSailPolicy raises first
    small = BatchedEnv(params, E, 3, 1)
    small.reset(full_batch(8301, E, 3, 1))
    small.use_torch_stream()
    with pytest.raises(_capi.EbcError, match="adult_num = 5") as ei:
        small.attach_sail(net)
    assert ei.value.code == _abi.ERR_INVALID
    _refused(small, K, _abi.ERR_STATE, "no network attached")
    with pytest.raises(ValueError, match="adult_num = 5"):
        DeviceSailPolicy(net).rollout(small, K, small.alloc_step_k_outputs(K, ("reward",)))
    # a network on another device
    if torch.cuda.device_count() > 1:
        other = SailNet(state_dict_of(5), device="cuda:1")
        with pytest.raises(_capi.EbcError, match="device") as ei:
            bare.attach_sail(other)
        assert ei.value.code == _abi.ERR_INVALID
        _refused(bare, K, _abi.ERR_STATE, "no network attached")
    # the refusals of ebc_step_k itself hold with the network attached
    env.set_human_actions(np.zeros((E, batch.N, 2)))
    with pytest.raises(_capi.EbcError, match="K") as ei:
        env.step_k(0, ("reward",), **SAIL)
    assert ei.value.code == _abi.ERR_INVALID
    _refused(env, K, _abi.ERR_UNSUPPORTED, "border", flags=_abi.FLAG_BORDER)
    _refused(env, K, _abi.ERR_UNSUPPORTED, "border", flags=_abi.FLAG_BORDER | ONE)
    for policy, name in ((_abi.HUMAN_LINEAR, "EBC_HUMAN_LINEAR"), (_abi.HUMAN_EXTERNAL, "EBC_HUMAN_EXTERNAL")):
        _refused(env, K, _abi.ERR_UNSUPPORTED, name, flags=ONE, human_policy=policy)
        twin = make_env(params, batch, net)
        twin.set_human_actions(np.zeros((E, batch.N, 2)))
        twin.step_k(K, ("reward",), human_policy=policy, robot_policy=_abi.ROBOT_SAIL)  # the per-step form takes it
    # beyond the kernel's LDS: adult_num 32 beside 40 rows.  UNSUPPORTED, never the per-step form, which takes the call
    big_net = SailNet(random_state_dict(32, 1), device=DEV)
    big = make_env(params, full_batch(8302, 3, 32, 8, walls=False), big_net)
    big.use_torch_stream()
    _refused(big, K, _abi.ERR_UNSUPPORTED, "48 KB of LDS", flags=ONE)
    assert b"per-step form" in _capi.lib().ebc_last_error()
    big.step_k(2, ("reward",), **SAIL)
    # a capturing stream
    outs = env.alloc_step_k_outputs(K, ("reward", "done"))
    side = torch.cuda.Stream()
    for flags in (AUTO, AUTO | ONE):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            env.use_torch_stream()
            env.step_k_device(outs, K, flags=flags, **SAIL)
            side.synchronize()
            graph.capture_begin()
            try:
                with pytest.raises(_capi.EbcError, match="captured") as ei:
                    env.step_k_device(outs, K, flags=flags, **SAIL)
                assert ei.value.code == _abi.ERR_UNSUPPORTED
            finally:
                graph.capture_end()
            env.step_k_device(outs, K, flags=flags, **SAIL)
            side.synchronize()
    env.synchronize()


# ------------------------------------------------------------------ 7. the evaluation in windows
def test_windowed_evaluation_gives_the_metrics_of_the_per_step_loop():
    """8 test cases of the golden run's env config with its weights: evaluate() with decide + step_device per step, and
    evaluate_windows() with 7 steps per call in either form, give the same dictionary."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy
    from ebcsim.train import evaluate, evaluate_windows
    z, meta, sd, _, _ = golden("sail_a5")
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["config_text"])
    sc = ebc_scene.SceneConfig.from_config(cfg)
    cases = 8
    batch = ebc_scene.SceneBatch.from_scenes([ebc_scene.generate_scene(sc, ebc_scene.COUNTER_OFFSET["test"] + c, "test")
                                              for c in range(cases)])
    assert batch.N + batch.S == 5
    params = params_of(z)
    params.time_limit = 6.0
    policy = DeviceSailPolicy(net_of(5))
    got = []
    for mode in ("loop", 0, ONE):
        env = BatchedEnv(params, cases, batch.N, batch.S)
        env.reset(batch)
        env.use_torch_stream()
        if mode == "loop":
            got.append(evaluate(env, lambda e: policy.decide(e)[0], 0.9, human_policy=_abi.HUMAN_ORCA))
        else:
            got.append(evaluate_windows(env, lambda e, K, outs: policy.rollout(e, K, outs, flags=mode), 0.9, 7))
        env.close()
    assert got[0]["num_episodes"] == cases and got[0]["timeout"] + got[0]["success"] <= cases
    assert got[1] == got[0] and got[2] == got[0], got
