"""ebc_step_k_world (-m gpu): the robot's FullState and the world-frame rows before every step of a K-step window, in the
per-step and the one-launch form.

The yardstick of the records is a twin env driven by the Python loop collect_sail_demos runs: robot_state_device,
observe_ob_device, row_counts_device, the robot's policy, step_device.  Everything is compared as raw bytes: (1) the
records of both forms against the loop's, every EbcStepKArgs output and the state left behind against plain ebc_step_k
on further twins, the two forms against each other; (2) partial requests between canaries, host and device location;
(3) refusals; (4) collect_sail_demos in windows against its loop; (5) the recorder filled by evaluate and by
evaluate_windows.

Shapes (the smallest that reach every path of the record stores): E = 5 and 37 with 1, 3 and 16 envs per workgroup, so
the last workgroup is partial and a run of records starts on and off a 16-byte boundary (9 doubles per env); ragged
scenes of 1..N humans and 0..S static rows at (N, S) = (3, 0) and (5, 2); T = 13 and 17; K = 1 and 7; a time limit of
three steps over an installed pool of scenes of other sizes, so every env restarts inside a K = 7 window."""
import ctypes as C

import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi, actions as ebc_actions, scene as ebc_scene
from helpers import Guarded
from sail_rollout_cases import full_batch, params_for, state_dict_of
from test_step_k_one_launch_gpu import KEYS9, _bytes_equal, _env, _state_equal, _synthetic_batch

pytestmark = pytest.mark.gpu

ONE, AUTO = _abi.FLAG_ONE_LAUNCH, _abi.FLAG_AUTO_RESET
WORLD = ("world_robot", "world_ob")
STEP_KEYS = ("reward", "done", "info", "dmin", "dist_to_goal", "robot_action_out", "obs_rotated")
LIMIT = 0.5  # seconds: the step taken at time 0.5, the third, is a Timeout
BIKES_LINEAR = (_abi.HUMAN_ORCA, _abi.HUMAN_LINEAR, _abi.HUMAN_ORCA)
_nets = {}


def _net(adult_num=5):
    from ebcsim.sail import SailNet
    if adult_num not in _nets:
        _nets[adult_num] = SailNet(state_dict_of(adult_num), device="cuda:0")
    return _nets[adult_num]


def _scenes(seed, E, N, S):
    """First scenes and an installed pool of E + 3 others, ragged in humans (1..N) and static rows (0..S)."""
    rs = np.random.RandomState(seed)
    first, pool = _synthetic_batch(rs, E, N, S, n_lo=1), _synthetic_batch(rs, E + 3, N, S, n_lo=1)
    assert len(set((pool.n_humans + pool.n_static).tolist())) > 1 or N + S == 1
    return first, pool


class Setup(object):
    """How every twin of a case is made: the scenes, the pool, the humans' table, the simulator, the network."""

    def __init__(self, params, first, pool, robot, sim=False, humans=_abi.HUMAN_ORCA, seed=5, K=7):
        self.params, self.first, self.pool, self.robot, self.sim, self.humans, self.K = params, first, pool, robot, sim, humans, K
        E = first.n
        self.ext = None
        if robot == "external":
            kin = "unicycle" if int(params.robot_kinematics) == _abi.UNICYCLE else "holonomic"
            space = ebc_actions.build_action_space(0.7) if kin == "holonomic" else ebc_actions.build_action_space(0.7, "unicycle")
            self.ext = np.ascontiguousarray(space[np.random.RandomState(seed).randint(len(space), size=(K, E))], dtype=np.float64)
        self.hact = np.random.RandomState(seed + 1).uniform(-0.4, 0.4, size=(E, first.N, 2))

    def env(self):
        g = _env(self.params, self.first.n, self.first.N, self.first.S)
        g.reset(self.first)
        g.set_scene_pool(self.pool)
        g.use_torch_stream()
        if self.humans == _abi.HUMAN_BY_TYPE:
            g.set_human_policies(*BIKES_LINEAR)
        if self.humans == _abi.HUMAN_EXTERNAL:
            g.set_human_actions(self.hact)
        if self.robot == "orca":
            g.robot_orca_sim(self.sim)
        if self.robot == "sail":
            g.attach_sail(_net())
        return g

    def kw(self, device=True):
        kw = dict(human_policy=self.humans)
        if self.robot == "orca":
            kw.update(robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)
        elif self.robot == "linear":
            kw.update(robot_policy=_abi.ROBOT_LINEAR)
        elif self.robot == "sail":
            kw.update(robot_policy=_abi.ROBOT_SAIL)
        else:
            kw.update(robot_policy=_abi.ROBOT_EXTERNAL, robot_action=torch.tensor(self.ext, device="cuda:0") if device else self.ext)
        return kw

    def loop(self, K, flags=AUTO):
        """The Python loop on a twin -> ({key: [K, ...]} on the host: the three records and the step's outputs, the env)"""
        from ebcsim.sail import DeviceSailPolicy
        g = self.env()
        E, R = g.E, g.R
        dev = torch.device("cuda", 0)
        rec = dict(world_robot=torch.zeros((K, E, 9), dtype=torch.float64, device=dev),
                   world_ob=torch.zeros((K, E, R, 5), dtype=torch.float64, device=dev),
                   n_rows=torch.zeros((K, E), dtype=torch.int64, device=dev))
        outs = [g.alloc_step_outputs(STEP_KEYS) for _ in range(K)]
        act = torch.zeros((E, 2), dtype=torch.float64, device=dev)
        ext = torch.tensor(self.ext, device=dev) if self.ext is not None else None
        pol = DeviceSailPolicy(_net()) if self.robot == "sail" else None
        for k in range(K):
            g.robot_state_device(rec["world_robot"][k])
            g.observe_ob_device(rec["world_ob"][k])
            g.row_counts_device(rec["n_rows"][k])
            if self.robot == "linear":
                g.step_device(outs[k], human_policy=self.humans, robot_policy=_abi.ROBOT_LINEAR, flags=flags)
                continue
            if self.robot == "orca":
                g.robot_orca_device(act, 0.15)
                a = act
            elif self.robot == "sail":
                a = pol.decide(g)[0]
            else:
                a = ext[k]
            g.step_device(outs[k], robot_action=a.contiguous(), human_policy=self.humans, flags=flags)
        g.synchronize()
        got = {k: v.cpu().numpy() for k, v in rec.items()}
        for name in STEP_KEYS:
            got[name] = np.stack([o[name].cpu().numpy() for o in outs])
        return got, g


def _window(g, K, keys, flags, kw):
    outs = g.alloc_step_k_outputs(K, keys)
    g.step_k_device(outs, K, flags=flags, **kw)
    g.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _check_case(s, K, both_forms=True, epg=None, monkeypatch=None):
    if epg is not None:
        monkeypatch.setenv("EBCSIM_ONE_LAUNCH_EPG", str(epg))
    want, L = s.loop(K)
    # rows past an env's own are zeros, in the yardstick itself
    rows = np.arange(L.R)[None, None, :] >= want["n_rows"][:, :, None]
    assert not want["world_ob"][rows].any() and (want["n_rows"] >= 1).all()
    if K > 3:  # the condition: every env ends at its third step at the latest and restarts inside the window
        assert want["done"][:K - 1].any(axis=0).all()
        P = s.pool.n
        for e in range(L.E):
            k = int(np.argmax(want["done"][:, e]))
            _bytes_equal(want["world_robot"][k + 1, e], s.pool.robot[e % P], "env %d: the record behind its terminal step %d" % (e, k))
            assert want["n_rows"][k + 1, e] == s.pool.n_humans[e % P] + s.pool.n_static[e % P]
        assert (want["n_rows"][0] != want["n_rows"][-1]).any()  # onto scenes of another size
    if int(s.params.robot_kinematics) == _abi.UNICYCLE:
        assert (np.diff(want["world_robot"][:3, :, 8], axis=0) != 0).any()  # the robot's theta moves
    keys = KEYS9 + WORLD
    got = {}
    for form, extra in (("per-step", 0), ("one-launch", ONE))[:2 if both_forms else 1]:
        g, plain = s.env(), s.env()
        got[form] = _window(g, K, keys, AUTO | extra, s.kw())
        ref = _window(plain, K, KEYS9, AUTO | extra, s.kw())
        for k in WORLD + ("n_rows",):
            _bytes_equal(got[form][k], want[k], "%s record %s against the Python loop" % (form, k))
        for k in STEP_KEYS:
            _bytes_equal(got[form][k], want[k], "%s output %s against the Python loop" % (form, k))
        for k in KEYS9:
            _bytes_equal(got[form][k], ref[k], "%s output %s against plain ebc_step_k" % (form, k))
        _state_equal(g, plain, s.robot == "orca" and s.sim, form + " against plain ebc_step_k:")
        _state_equal(g, L, s.robot == "orca" and s.sim, form + " against the Python loop:")
    if both_forms:
        for k in keys:
            _bytes_equal(got["per-step"][k], got["one-launch"][k], "the two forms, " + k)


# ------------------------------------------------------------------ 1. the records, every output, the state left behind
# (id, E, N, S, T, K, robot, persistent simulator, humans, envs per workgroup)
CASES = [
    ("orca-sim-E37-5+2-T17-epg3", 37, 5, 2, 17, 7, "orca", True, _abi.HUMAN_ORCA, 3),
    ("orca-E37-5+2-T13-epg16", 37, 5, 2, 13, 7, "orca", False, _abi.HUMAN_ORCA, 16),
    ("orca-sim-E5-3+0-T17-K1-epg1", 5, 3, 0, 17, 1, "orca", True, _abi.HUMAN_ORCA, 1),
    ("linear-E5-3+0-T17-epg1", 5, 3, 0, 17, 7, "linear", False, _abi.HUMAN_ORCA, 1),
    ("linear-E37-5+2-T13-by-type-epg16", 37, 5, 2, 13, 7, "linear", False, _abi.HUMAN_BY_TYPE, 16),
    ("external-E5-3+0-T13-K1-epg3", 5, 3, 0, 13, 1, "external", False, _abi.HUMAN_ORCA, 3),
    ("external-E37-3+0-T17-by-type-epg3", 37, 3, 0, 17, 7, "external", False, _abi.HUMAN_BY_TYPE, 3),
    ("external-E37-5+2-T13-epg1", 37, 5, 2, 13, 7, "external", False, _abi.HUMAN_ORCA, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_records_outputs_and_state_three_robots(case, monkeypatch):
    tag, E, N, S, T, K, robot, sim, humans, epg = case
    first, pool = _scenes(100 + CASES.index(case), E, N, S)
    _check_case(Setup(params_for(T, time_limit=LIMIT), first, pool, robot, sim, humans, K=K), K, epg=epg, monkeypatch=monkeypatch)


def test_cases_cover_the_shapes():
    col = lambda i: {c[i] for c in CASES}  # noqa: E731
    assert col(1) == {5, 37} and {(c[2], c[3]) for c in CASES} == {(3, 0), (5, 2)} and col(4) == {13, 17} and col(5) == {1, 7}
    assert col(9) == {1, 3, 16} and col(6) == {"orca", "linear", "external"} and {c[7] for c in CASES if c[6] == "orca"} == {True, False}
    assert col(8) == {_abi.HUMAN_ORCA, _abi.HUMAN_BY_TYPE}


def test_unicycle_external_rotations(monkeypatch):
    first, pool = _scenes(300, 37, 5, 2)
    _check_case(Setup(params_for(17, _abi.UNICYCLE, time_limit=LIMIT), first, pool, "external"), 7, epg=3, monkeypatch=monkeypatch)


@pytest.mark.parametrize("humans", [_abi.HUMAN_LINEAR, _abi.HUMAN_EXTERNAL], ids=["linear", "external"])
def test_linear_and_external_humans_per_step_form(humans):
    first, pool = _scenes(400 + humans, 37, 5, 2)
    _check_case(Setup(params_for(13, time_limit=LIMIT), first, pool, "linear", humans=humans), 7, both_forms=False)


@pytest.mark.parametrize("humans", [_abi.HUMAN_ORCA, _abi.HUMAN_BY_TYPE], ids=["orca", "by-type"])
def test_sail_robot(humans, monkeypatch):
    """EBC_ROBOT_SAIL: scenes of exactly adult_num = 5 rows; the loop decides with DeviceSailPolicy.decide."""
    first, pool = full_batch(500, 37, 5, 0), full_batch(501, 40, 5, 0, arrived=False)
    s = Setup(params_for(17, time_limit=LIMIT), first, pool, "sail", humans=humans)
    monkeypatch.setenv("EBCSIM_ONE_LAUNCH_EPG", "3")
    want, L = s.loop(7)
    assert np.isfinite(want["robot_action_out"]).all() and want["done"][:6].any(axis=0).all()
    keys = KEYS9 + WORLD
    got = {}
    for form, extra in (("per-step", 0), ("one-launch", ONE)):
        g, plain = s.env(), s.env()
        got[form] = _window(g, 7, keys, AUTO | extra, s.kw())
        ref = _window(plain, 7, KEYS9, AUTO | extra, s.kw())
        for k in WORLD + ("n_rows",) + STEP_KEYS:
            _bytes_equal(got[form][k], want[k], "%s %s against the Python loop" % (form, k))
        for k in KEYS9:
            _bytes_equal(got[form][k], ref[k], "%s %s against plain ebc_step_k" % (form, k))
        _state_equal(g, plain, False, form)
    for k in keys:
        _bytes_equal(got["per-step"][k], got["one-launch"][k], "the two forms, " + k)


# ------------------------------------------------------------------ 2. partial requests, bounds, host and device
@pytest.mark.parametrize("keys", [("world_robot",), ("world_ob",), ("world_robot", "reward"), ("world_ob", "state_rotated"),
                                  ("world_robot", "world_ob"), KEYS9 + WORLD], ids=lambda k: "+".join(k) if len(k) < 4 else "all")
def test_partial_requests_stay_inside_their_buffers(keys, monkeypatch):
    """Every output a slice of a canary-filled tensor, poisoned inside: all of it written, nothing beside it; the two
    forms equal; the host-location calls equal the device-location calls; the state is plain ebc_step_k's."""
    first, pool = _scenes(600, 37, 5, 2)
    s = Setup(params_for(17, time_limit=LIMIT), first, pool, "orca", True)
    monkeypatch.setenv("EBCSIM_ONE_LAUNCH_EPG", "3")
    K = 7
    want, _ = s.loop(K)
    a, b, ha, hb, plain = s.env(), s.env(), s.env(), s.env(), s.env()
    shapes = a._STEP_K_SHAPES(a.E, a.R, a.T)
    ga, gb = ({k: Guarded((K,) + shapes[k][0], getattr(torch, shapes[k][1]), tile_rows=1) for k in keys} for _ in range(2))
    a.step_k_device({k: g.t for k, g in ga.items()}, K, flags=AUTO, **s.kw())
    b.step_k_device({k: g.t for k, g in gb.items()}, K, flags=AUTO | ONE, **s.kw())
    a.synchronize()
    b.synchronize()
    host_a = ha.step_k(K, keys, flags=AUTO, **s.kw(device=False))
    host_b = hb.step_k(K, keys, flags=AUTO | ONE, **s.kw(device=False))
    plain.step_k(K, ("reward",), flags=AUTO, **s.kw(device=False))
    for k in keys:
        x, y = ga[k].check(), gb[k].check()
        _bytes_equal(x, y, "the two forms, device, " + k)
        _bytes_equal(host_a[k], x, "host per-step " + k)
        _bytes_equal(host_b[k], x, "host one-launch " + k)
        if k in want:
            _bytes_equal(x, want[k], k + " against the Python loop")
    for g in (a, b, ha, hb):
        _state_equal(g, plain, True, "partial request")


# ------------------------------------------------------------------ 3. refusals
def _raw_call(env, K, flags, robot, ob, struct_size=None, reserved=0):
    a = env._step_k_args(K, _abi.DEVICE, {}, _abi.HUMAN_ORCA, _abi.ROBOT_LINEAR, flags, 0.0, None)
    w = _abi.EbcStepKWorld()
    w.struct_size = C.sizeof(w) if struct_size is None else struct_size
    w.reserved, w.robot, w.ob = reserved, robot, ob
    return env._L.ebc_step_k_world(env._h, C.addressof(a), C.addressof(w)), env._L.ebc_last_error().decode()


def test_refusals():
    first, pool = _scenes(700, 5, 3, 0)
    params = params_for(17, time_limit=LIMIT)
    env = _env(params, 5, 3, 0)
    K = 4
    lin = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR)
    for flags in (0, ONE):
        with pytest.raises(_capi.EbcError, match="ebc_step_k_world before ebc_reset") as ei:
            env.step_k(K, ("world_robot",), flags=flags, **lin)
        assert ei.value.code == _abi.ERR_STATE
    env.reset(first)
    env.set_scene_pool(pool)
    env.use_torch_stream()
    env.set_human_actions(np.zeros((5, 3, 2)))
    before = env.get_state()
    shapes = env._STEP_K_SHAPES(env.E, env.R, env.T)
    g = {k: Guarded((K,) + shapes[k][0], getattr(torch, shapes[k][1]), tile_rows=1) for k in WORLD + ("reward",)}
    outs = {k: v.t for k, v in g.items()}

    def refused(code, match, **kw):
        with pytest.raises(_capi.EbcError, match=match) as ei:
            env.step_k_device(outs, kw.pop("K", K), **kw)
        assert ei.value.code == code, match

    for policy, name in ((_abi.HUMAN_LINEAR, "EBC_HUMAN_LINEAR"), (_abi.HUMAN_EXTERNAL, "EBC_HUMAN_EXTERNAL")):
        refused(_abi.ERR_UNSUPPORTED, "ebc_step_k_world: EBC_FLAG_ONE_LAUNCH with " + name, flags=AUTO | ONE, human_policy=policy,
                robot_policy=_abi.ROBOT_LINEAR)
    for flags in (0, ONE):
        with pytest.raises(_capi.EbcError, match="K") as ei:
            env.step_k(0, ("world_ob",), flags=flags, **lin)
        assert ei.value.code == _abi.ERR_INVALID
        refused(_abi.ERR_UNSUPPORTED, "ebc_step_k_world: no border", flags=flags | _abi.FLAG_BORDER, **lin)
    # the side struct's own
    rp, op = outs["world_robot"].data_ptr(), outs["world_ob"].data_ptr()
    for (rc, msg), name in ((_raw_call(env, K, 0, None, None), "both NULL"), (_raw_call(env, K, ONE, rp, op, struct_size=16), "EbcStepKWorld.struct_size"),
                            (_raw_call(env, K, 0, rp, op, reserved=7), "EbcStepKWorld.reserved")):
        assert rc == _abi.ERR_INVALID and name in msg, (rc, msg)
    with pytest.raises(ValueError, match="do not go together"):
        from ebcsim.occupancy import OccupancySpec
        om = OccupancySpec(cell_num=4, cell_size=1.0, channels=3)
        wide = env.alloc_step_k_outputs(K, ("state_wide",), om=om)
        env.step_k_device(dict(outs, **wide), K, om=om, **lin)
    # a capturing stream
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        env.use_torch_stream()
        side.synchronize()
        graph.capture_begin()
        try:
            for flags in (AUTO, AUTO | ONE):
                refused(_abi.ERR_UNSUPPORTED, "ebc_step_k_world: the stream is being captured", flags=flags, **lin)
        finally:
            graph.capture_end()
        side.synchronize()
    env.synchronize()
    for v in g.values():
        v.check(written=False)  # nothing was written by a refused call
    after = env.get_state()
    for k in before:
        _bytes_equal(before[k], after[k], "state after the refused calls: " + k)
    env.step_k_device(outs, K, flags=AUTO | ONE, **lin)  # and the handle still takes the call
    env.synchronize()
    for v in g.values():
        v.check()


# ------------------------------------------------------------------ 4. collect_sail_demos in windows
def _near_goal_batch(E, N, shift):
    """Robot e a metre under its goal, which it reaches at 0.7 m/s within six steps; its humans 3 m and more to the side,
    walking away from it: nothing decides an episode but the arrival."""
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = ebc_scene.SceneBatch(E, N, 0, np.full(E, N, np.int32), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                             f(E, N), np.zeros((E, N), np.uint8), np.zeros(E, np.int32), f(E, 1), f(E, 1), f(E, 1), None, f(E, 9))
    for e in range(E):
        rx = 0.2 * e + shift
        b.robot[e] = [rx, -0.5, 0, 0, 0.3, rx + 0.05 * e, 0.5 + 0.02 * e, 0.7, np.pi / 2]
        for i in range(N):
            side = 1.0 if i % 2 else -1.0
            b.px[e, i], b.py[e, i] = rx + side * (3.0 + 0.4 * i), -0.5 + 0.3 * i
            b.vx[e, i], b.vy[e, i] = side * 0.3, 0.0
            b.gx[e, i], b.gy[e, i] = rx + side * 6.0, -0.5 + 0.3 * i
            b.radius[e, i], b.v_pref[e, i] = 0.25 + 0.01 * i, 0.8
    return b


@pytest.mark.parametrize("one_launch", [False, True], ids=["per-step", "one-launch"])
def test_collect_sail_demos_in_windows_is_the_loop(one_launch):
    from ebcsim.sail_train import collect_sail_demos
    E, N, steps = 6, 3, 12
    params = params_for(17, time_limit=4.0)
    got = []
    for kw in (dict(), dict(steps_per_call=5, one_launch=one_launch)):  # windows of 5, 5 and 2 steps
        env = _env(params, E, N, 0)
        env.reset(_near_goal_batch(E, N, 0.0))
        env.set_scene_pool(_near_goal_batch(E + 1, N, 0.07))
        env.use_torch_stream()
        got.append(collect_sail_demos(env, steps, **kw))
        env.synchronize()
    loop, win = got
    assert loop["steps"] > 0 and loop["episodes"] >= E  # kept samples, and every env restarted inside the window
    assert set(win) == set(loop) and win["steps"] == loop["steps"] and win["episodes"] == loop["episodes"]
    for k in ("robot", "ob", "n_rows", "target"):
        _bytes_equal(win[k].cpu().numpy(), loop[k].cpu().numpy(), k)


# ------------------------------------------------------------------ 5. the recorder
def test_recorder_filled_by_evaluate_and_by_windows(tmp_path):
    from ebcsim.record import EpisodeRecorder
    from ebcsim.sail import DeviceSailPolicy
    from ebcsim.train import evaluate, evaluate_windows
    E = 6
    params = params_for(17, time_limit=2.0)  # 8 steps and the Timeout step
    batch = full_batch(800, E, 5, 0)
    pol = DeviceSailPolicy(_net())
    eps, metrics, recs = [], [], []
    for mode in ("loop", "windows", "one-launch"):
        env = _env(params, E, 5, 0)
        env.reset(batch)
        env.use_torch_stream()
        rec = EpisodeRecorder(env, 10)
        if mode == "loop":
            m = evaluate(env, lambda e: pol.decide(e)[0], 0.9, record=rec)
        else:
            flags = ONE if mode == "one-launch" else 0
            m = evaluate_windows(env, rec.recording(lambda e, K, outs: pol.rollout(e, K, outs, flags=flags)), 0.9, 4)
        eps.append(rec.episodes())
        metrics.append({k: v for k, v in m.items()})
        recs.append(rec)
    for other in eps[1:]:
        assert set(other) == set(eps[0]) == {"robot", "ob", "n_rows", "length", "final"}
        for k in eps[0]:
            _bytes_equal(other[k], eps[0][k], "recorder " + k)
    assert metrics[0] == metrics[1] == metrics[2]
    ep, dt = eps[0], float(params.time_step)
    end_time = recs[0].end_time  # the tally's, handed over by evaluate()
    assert (ep["final"] >= 0).all() and (ep["length"] >= 1).all()
    for e in range(E):
        n = int(ep["length"][e])
        if ep["final"][e] == _abi.INFO_TIMEOUT:
            assert end_time[e] == 2.0 and (n - 1) * dt >= 2.0 > (n - 2) * dt
        else:
            assert end_time[e] == n * dt
        assert (ep["n_rows"][:n, e] == 5).all() and not ep["n_rows"][n:, e].any()
        assert not ep["robot"][n:, e].any() and not ep["ob"][n:, e].any() and ep["robot"][:n, e, 4].all()
    _bytes_equal(ep["robot"][0], batch.robot, "the first record is the reset scene's robot")
    path = recs[0].save(str(tmp_path / "episodes.npz"))
    z = np.load(path)
    assert set(z.files) >= {"robot", "ob", "n_rows", "length", "final", "type", "case"}
    _bytes_equal(z["ob"], ep["ob"], "saved ob")
    np.testing.assert_array_equal(z["type"], batch.type)
    np.testing.assert_array_equal(z["case"], np.arange(E))
