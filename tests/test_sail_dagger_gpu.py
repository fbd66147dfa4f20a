"""ebc_sail_dagger_k and the DAgger schedule (-m gpu).  (1) one call is the composition of the entries it replaces, in
bytes, for every case of tests/sail_dagger_cases.py; (2) its two ends are ebc_step_k with EBC_ROBOT_SAIL and with
EBC_ROBOT_ORCA; (3) a NaN action of the learner reaches nothing when the expert acts; (4) every output between canaries;
(5) refusals; (6) the schedule.  tests/test_sail_dagger_cpu.py walks the same cases on the oracle."""
import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi, sail_train
from helpers import Guarded
from sail_dagger_cases import AUTO, CASES, OUT, SAFETY, SCHEDULE, oracle_walk, schedule_setup, setup
from sail_rollout_cases import KEYS9, full_batch, params_for, state_dict_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAIL = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_SAIL)
_nets = {}


def net_of(adult_num):
    from ebcsim.sail import SailNet
    if adult_num not in _nets:
        _nets[adult_num] = SailNet(state_dict_of(adult_num), device=DEV)
    return _nets[adult_num]


def make_env(params, batch, net, pool=None, sim=False):
    from ebcsim.batched import BatchedEnv
    env = BatchedEnv(params, batch.n, batch.N, batch.S)
    env.reset(batch)
    if pool is not None:
        env.set_scene_pool(pool)
    if net is not None:
        env.attach_sail(net)
    if sim:
        env.robot_orca_sim(True)
    env.use_torch_stream()
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


def _mask_dev(mask):
    return None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)


def _dagger(env, K, mask, flags=0, optional=("reward", "done", "info"), safety=SAFETY):
    out = env.alloc_sail_dagger_outputs(K, optional)
    env.sail_dagger_k_device(out, K, take_expert=_mask_dev(mask), safety_space=safety, flags=flags)
    env.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. bytes of the composition
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_one_call_is_the_composition_in_bytes(case):
    from ebcsim.sail import DeviceSailPolicy
    tag, A, humans, static, T, E, K, flags, pool_n, sim, kind = case
    params, batch, pool, sd, mask = setup(case)
    net = net_of(A)
    a, b = make_env(params, batch, net, pool, sim), make_env(params, batch, net, pool, sim)
    assert a.T == T and a.R == A and a.E == E
    got = _dagger(a, K, mask, flags)
    pol = DeviceSailPolicy(net)
    m = _mask_dev(mask)
    robot = torch.empty((E, 9), dtype=torch.float64, device=DEV)
    ob = torch.empty((E, A, 5), dtype=torch.float64, device=DEV)
    n_rows = torch.empty((E,), dtype=torch.int64, device=DEV)
    expert = torch.empty((E, 2), dtype=torch.float64, device=DEV)
    so = b.alloc_step_outputs(("reward", "done", "info"))
    for k in range(K):
        b.robot_state_device(robot)
        b.observe_ob_device(ob)
        b.row_counts_device(n_rows)
        learner, _ = pol.decide(b)
        b.robot_orca_device(expert, SAFETY)
        act = learner.clone() if m is None else torch.where(m[k].bool()[:, None], expert, learner).contiguous()
        b.step_device(so, robot_action=act, human_policy=_abi.HUMAN_ORCA, flags=flags)
        b.synchronize()
        want = dict(robot=robot, ob=ob, n_rows=n_rows, learner_action=learner, expert_action=expert, robot_action_out=act, **so)
        for name in OUT:
            _bytes_equal(got[name][k], want[name].cpu().numpy(), "%s step %d %s" % (tag, k, name))
    assert np.isfinite(got["robot_action_out"]).all() and (got["n_rows"] == A).all()
    if flags and K == 20:
        assert int(got["done"].sum()) > E
    # the oracle's walk of the same case: the masks (row counts, and the terminal steps where the actions agree)
    walk = oracle_walk(case)[0]
    np.testing.assert_array_equal(got["n_rows"], walk["n_rows"])
    _state_equal(a, b, tag)
    if sim:
        sa, sb = a.robot_orca_sim_state(), b.robot_orca_sim_state()
        for name in sa:
            _bytes_equal(sa[name], sb[name], "%s simulator %s" % (tag, name))
    # five further steps: what they compute shows the tile, the grid slot, the pool cursor and the simulators
    more = dict(SAIL) if not sim else dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, robot_safety_space=SAFETY)
    ca, cb = a.step_k(5, KEYS9, flags=flags, **more), b.step_k(5, KEYS9, flags=flags, **more)
    for name in KEYS9:
        _bytes_equal(ca[name], cb[name], "%s continuation %s" % (tag, name))


# ------------------------------------------------------------------ 2. the two ends
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=lambda c: c[0])
def test_the_two_ends_are_step_k(case):
    tag, A, humans, static, T, E, K, flags, pool_n, sim, kind = case
    params, batch, pool, sd, _ = setup(case)
    net = net_of(A)
    keys = ("n_rows", "robot_action_out", "reward", "done", "info")
    ref = make_env(params, batch, net, pool, sim)
    want = ref.step_k(K, keys, flags=flags, **SAIL)
    for name, mask in (("NULL", None), ("zeros", np.zeros((K, E), np.uint8))):
        env = make_env(params, batch, net, pool, sim)
        got = _dagger(env, K, mask, flags)
        for k in keys:
            _bytes_equal(got[k], want[k], "%s mask %s: %s against EBC_ROBOT_SAIL" % (tag, name, k))
        _bytes_equal(got["learner_action"], want["robot_action_out"], "%s mask %s: learner" % (tag, name))
        _state_equal(env, ref, "%s mask %s" % (tag, name))
    ref = make_env(params, batch, net, pool, sim)
    want = ref.step_k(K, keys, flags=flags, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, robot_safety_space=SAFETY)
    env = make_env(params, batch, net, pool, sim)
    got = _dagger(env, K, np.ones((K, E), np.uint8), flags)
    for k in ("robot_action_out", "reward", "done", "info"):
        _bytes_equal(got[k], want[k], "%s mask ones: %s against EBC_ROBOT_ORCA" % (tag, k))
    _bytes_equal(got["expert_action"], want["robot_action_out"], "%s mask ones: expert" % tag)
    _state_equal(env, ref, "%s mask ones" % tag)
    if sim:
        sa, sb = env.robot_orca_sim_state(), ref.robot_orca_sim_state()
        for name in sa:
            _bytes_equal(sa[name], sb[name], "%s mask ones: simulator %s" % (tag, name))


# ------------------------------------------------------------------ 3. a NaN of the learner reaches nothing
def test_nan_learner_action_reaches_nothing_when_the_expert_acts():
    E, K, A, bad = 9, 8, 5, 4
    params = params_for(17)
    good = full_batch(9500, E, A, 0)
    broken = full_batch(9500, E, A, 0)
    broken.n_humans[bad] = A - 1
    mask = (np.random.RandomState(9501).uniform(size=(K, E)) < 0.5).astype(np.uint8)
    mask[:, bad] = 1
    net = net_of(A)
    got = _dagger(make_env(params, broken, net), K, mask)
    ref = _dagger(make_env(params, good, net), K, mask)
    assert (got["n_rows"][:, bad] == A - 1).all() and np.isnan(got["learner_action"][:, bad]).all()
    assert np.isfinite(got["expert_action"]).all()
    _bytes_equal(got["robot_action_out"][:, bad], got["expert_action"][:, bad], "the defective env executes its expert's action")
    assert np.isfinite(got["robot_action_out"]).all() and np.isfinite(got["reward"]).all()
    others = [e for e in range(E) if e != bad]
    assert mask[:, others].any() and not mask[:, others].all()
    for name in OUT:
        _bytes_equal(got[name][:, others], ref[name][:, others], "the other envs' %s" % name)


# ------------------------------------------------------------------ 4. every output between canaries
def _guarded(env, K, keys):
    shapes = env._DAGGER_SHAPES(env.E, env.R)
    return {k: Guarded((K,) + shapes[k][0], getattr(torch, shapes[k][1]), tile_rows=1) for k in keys}


@pytest.mark.parametrize("optional", [("reward", "done", "info"), ()], ids=["with-optional", "required-only"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=lambda c: c[0])
def test_outputs_stay_inside_their_buffers(case, optional):
    tag, A, humans, static, T, E, K, flags, pool_n, sim, kind = case
    params, batch, pool, sd, mask = setup(case)
    net = net_of(A)
    a, b = make_env(params, batch, net, pool, sim), make_env(params, batch, net, pool, sim)
    keys = a._DAGGER_REQUIRED + tuple(optional)
    g = _guarded(a, K, keys)
    a.sail_dagger_k_device({k: v.t for k, v in g.items()}, K, take_expert=_mask_dev(mask), safety_space=SAFETY, flags=flags)
    a.synchronize()
    want = _dagger(b, K, mask, flags, optional)
    for k in keys:
        _bytes_equal(g[k].check(), want[k], "%s guarded %s" % (tag, k))
    _state_equal(a, b, tag + " guarded")


# ------------------------------------------------------------------ 5. refusals
def _refused(env, K, code, match, flags=0, drop=None, safety=SAFETY, struct_size=None):
    """A refused call: the code, the message, guarded outputs untouched, state bytes untouched."""
    before = env.get_state()
    g = _guarded(env, max(K, 1), OUT)
    outs = {k: v.t for k, v in g.items() if k != drop}
    with pytest.raises(_capi.EbcError, match=match) as ei:
        if struct_size is None and K >= 1:
            env.sail_dagger_k_device(outs, K, safety_space=safety, flags=flags)
        else:  # what the wrapper's own shape checks would stop
            _raw(env, outs, K, safety, flags, struct_size)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    env.synchronize()
    for v in g.values():
        v.check(written=False)
    after = env.get_state()
    for k in before:
        _bytes_equal(before[k], after[k], "state after a refused call: " + k)


def _raw(env, outs, K, safety, flags, struct_size=None):
    """The entry itself, past the checks of sail_dagger_k_device."""
    import ctypes as C
    a = _abi.EbcSailDaggerArgs()
    a.struct_size = C.sizeof(a) if struct_size is None else struct_size
    a.K, a.human_policy, a.flags, a.expert_safety_space = K, _abi.HUMAN_ORCA, flags, safety
    for k, t in outs.items():
        setattr(a, k, t.data_ptr())
    _capi.check(_capi.lib().ebc_sail_dagger_k(env._h, C.addressof(a)))


def test_refusals():
    from ebcsim.batched import BatchedEnv
    E, K = 8, 4
    params = params_for(17)
    batch = full_batch(9600, E, 5, 0)
    net = net_of(5)
    # before reset
    fresh = BatchedEnv(params, E, batch.N, batch.S)
    fresh.attach_sail(net)
    with pytest.raises(_capi.EbcError, match="before ebc_reset") as ei:
        fresh.sail_dagger_k_device(fresh.alloc_sail_dagger_outputs(K), K)
    assert ei.value.code == _abi.ERR_STATE
    # no network attached: never, and after a detach
    bare = make_env(params, batch, None)
    _refused(bare, K, _abi.ERR_STATE, "no network attached")
    bare.attach_sail(net)
    _dagger(bare, K, None)
    bare.attach_sail(None)
    _refused(bare, K, _abi.ERR_STATE, "no network attached")
    # the conditions and wording of check_robot_orca
    uni = make_env(params_for(17, _abi.UNICYCLE), batch, net)
    _refused(uni, K, _abi.ERR_UNSUPPORTED, "holonomic robots only")
    wide = make_env(params, full_batch(9601, 3, 32, 1, walls=False), net_of(32))
    _refused(wide, K, _abi.ERR_UNSUPPORTED, "more than 32 observation rows")
    env = make_env(params, batch, net)
    for safety in (-0.1, float("nan")):
        _refused(env, K, _abi.ERR_INVALID, "safety_space", safety=safety)
    # the forms that are not built
    _refused(env, K, _abi.ERR_UNSUPPORTED, "EBC_FLAG_ONE_LAUNCH", flags=_abi.FLAG_ONE_LAUNCH)
    _refused(env, K, _abi.ERR_UNSUPPORTED, "EBC_FLAG_ONE_LAUNCH", flags=_abi.FLAG_ONE_LAUNCH | AUTO)
    _refused(env, K, _abi.ERR_UNSUPPORTED, "border", flags=_abi.FLAG_BORDER)
    # arguments
    _refused(env, 0, _abi.ERR_INVALID, "K")
    _refused(env, -3, _abi.ERR_INVALID, "K")
    for name in BatchedEnv._DAGGER_REQUIRED:
        _refused(env, K, _abi.ERR_INVALID, "required output is NULL", drop=name)
    _refused(env, K, _abi.ERR_INVALID, "struct_size", struct_size=96)
    # a capturing stream
    outs = env.alloc_sail_dagger_outputs(K)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        env.use_torch_stream()
        env.sail_dagger_k_device(outs, K, flags=AUTO)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError, match="captured") as ei:
                env.sail_dagger_k_device(outs, K, flags=AUTO)
            assert ei.value.code == _abi.ERR_UNSUPPORTED
        finally:
            graph.capture_end()
        env.sail_dagger_k_device(outs, K, flags=AUTO)
        side.synchronize()
    env.synchronize()
    # the refused calls left a working handle behind
    env.use_torch_stream()
    got = _dagger(env, K, None)
    assert np.isfinite(got["robot_action_out"]).all()


# ------------------------------------------------------------------ 6. the schedule
def test_dagger_schedule(tmp_path):
    from ebcsim.sail import DeviceSailPolicy, SailModule
    c = SCHEDULE
    params, batch, sd = schedule_setup()
    E, A = c["E"], 5
    trainer = sail_train.SailTrainer(sd, device=DEV, optimizer="adam", lr=1e-3)
    env = make_env(params, batch, trainer.net)
    start = trainer.flat.detach().clone()
    rounds, capacity = [], 2000
    gen = torch.Generator(device=DEV).manual_seed(3)
    losses, data = sail_train.dagger(env, trainer, c["rounds"], c["demo_steps"], c["dagger_steps"], c["epochs"], c["epochs"], 256,
                                     capacity=capacity, generator=gen, safety_space=SAFETY, on_round=lambda i, info: rounds.append(info))
    assert [r["round"] for r in rounds] == [0, 1, 2] and [r["beta"] for r in rounds] == [1.0, 0.5, 0.25]
    assert len(losses) == 3 and all(len(x) == c["epochs"] and np.isfinite(x).all() for x in losses)
    # the aggregate grows and respects its capacity
    total = sum(r["samples"] for r in rounds)
    agg = [r["aggregate"] for r in rounds]
    print("samples per round %s, aggregate %s" % ([r["samples"] for r in rounds], agg))
    assert rounds[0]["samples"] > 0 and all(r["samples"] > 0 for r in rounds[1:])
    assert agg[1] > agg[0] and agg[2] >= agg[1] and max(agg) <= capacity and agg[2] == min(capacity, total) == len(data)
    assert total > capacity  # the capacity did cut
    # the weights change
    assert not torch.equal(start, trainer.flat.detach())
    # one more window: what it keeps, and whose weights decide
    pol = DeviceSailPolicy(trainer.net)
    first = pol.decide(env)[0].clone()
    got = sail_train.collect_dagger(env, 6, 0.5, torch.Generator(device=DEV).manual_seed(4), SAFETY)
    win = got["window"]
    _bytes_equal(win["learner_action"][0].cpu().numpy(), first.cpu().numpy(), "the window's first decisions are the new weights'")
    keep = got["keep"]
    assert got["steps"] == int(keep.sum()) > 0 and tuple(got["robot"].shape) == (got["steps"], 9)
    assert bool(sail_train.live_envs(got["robot"], got["n_rows"], None, A).all())  # every kept sample is live
    assert bool(torch.isfinite(got["target"]).all())
    flat = lambda t: t.reshape(6 * E, -1)[keep].cpu().numpy()  # noqa: E731
    _bytes_equal(got["target"].cpu().numpy(), flat(win["expert_action"]), "target = the expert's action at the kept indices")
    _bytes_equal(got["executed"].cpu().numpy(), flat(win["robot_action_out"]), "executed")
    _bytes_equal(got["learner"].cpu().numpy(), flat(win["learner_action"]), "learner")
    _bytes_equal(got["robot"].cpu().numpy(), flat(win["robot"]), "robot")
    live_all = sail_train.live_envs(win["robot"].reshape(6 * E, 9), win["n_rows"].reshape(-1), None, A)
    assert torch.equal(keep, live_all & torch.isfinite(win["expert_action"].reshape(6 * E, 2)).all(dim=1))
    take = got["take_expert"]
    assert take.dtype == torch.bool and bool(take.any()) and not bool(take.all())
    assert got["episodes"] == int(win["done"].sum()) and got["success"] + got["collision"] + got["timeout"] == got["episodes"]
    # the saved file
    path = str(tmp_path / "sail_dagger.pth")
    trainer.save(path)
    SailModule(A).load_state_dict(torch.load(path), strict=True)
    env.close()
