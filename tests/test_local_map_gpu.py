"""The angular local map on the device (ebc_local_map, ebc_step_with_map; -m gpu).

Against the reference's own maps (tests/golden/local_map.npz, local_map_edges.npz), against the host build of the same
source (tests/native/local_map_host.cc) on device-generated scenes, through auto-reset and pool re-installs, and the
refusals of the C ABI.  A canary on each side of the map buffers checks that the kernel writes [E][dim] and no more."""
import configparser
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi, config as ebc_config, scene as ebc_scene
from helpers import GOLDEN, Guarded
from test_local_map_cpu import (ROOT, _bench_scene_cfg, _bits_equal, _build, _check_pose, _fixture_cases,
                                _static_known_answer)

pytestmark = pytest.mark.gpu
PI = np.pi


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return _build(tmp_path_factory, "local_map_host_gpu", "local_map_host.cc")


def _host_maps(lib, polys, n_poly, robot, dim, max_range=3.0, amin=-PI, amax=PI, normalize=True):
    out = np.zeros((len(robot), dim))
    for e in range(len(robot)):
        poly = np.ascontiguousarray(polys[e, :max(n_poly[e], 1)])
        pose = np.ascontiguousarray([robot[e, 0], robot[e, 1], robot[e, 4], robot[e, 8]])
        row = np.zeros(dim)
        lib.local_map_host(C.c_void_p(poly.ctypes.data), int(n_poly[e]), C.c_void_p(pose.ctypes.data), 1, dim,
                           C.c_double(max_range), C.c_double(amin), C.c_double(amax), int(normalize),
                           C.c_void_p(row.ctypes.data))
        out[e] = row
    return out


def _atan2_tie(lib, poly, pose, dim=48, amin=-PI, amax=PI, tol=1e-9):
    """Whether some (vertex, corner) sector quotient (atan2(ry, rx) - angle_min) / res of this pose lies within `tol` of
    an integer: there the device's atan2 (ocml) and the host's (libm) may round to neighbouring doubles that truncate
    to different sectors.  Generated scenes sit on a 0.1 grid and start at theta = pi / 2, so 45-degree offsets, which
    land exactly on a sector boundary of dim 48, are common: about 0.4 % of envs at the first step."""
    c, s = C.c_double(), C.c_double()
    lib.sincos_dd_host(C.c_double(pose[3]), C.byref(c), C.byref(s))
    res = (amax - amin) / dim
    for v in np.asarray(poly).reshape(-1, 2):
        for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
            dx, dy = v[0] - (pose[0] + sx * pose[2]), v[1] - (pose[1] + sy * pose[2])
            q = (np.arctan2(dy * c.value - dx * s.value, dx * c.value + dy * s.value) - amin) / res
            if abs(q - round(q)) < tol:
                return True
    return False


def _assert_device_equals_host(lib, dev, host, polys, n_poly, robot, what):
    """Bit for bit, except envs whose pose puts a sector quotient on an integer (_atan2_tie): every other env must match.
    Measured at the generated start pose (theta = pi / 2, obstacles on the 0.1 grid): 17 of 4096 envs differ with 4 walls,
    45 of 4096 with 20 polygons; the bound below is 2.5 %."""
    bad = np.nonzero((dev.view(np.uint64) != host.view(np.uint64)).any(1))[0]
    for e in bad:
        pose = [robot[e, 0], robot[e, 1], robot[e, 4], robot[e, 8]]
        assert _atan2_tie(lib, polys[e, :n_poly[e]], pose), "%s: env %d differs without an atan2 tie" % (what, e)
    assert len(bad) <= max(1, len(dev) // 40), "%s: %d envs on atan2 ties" % (what, len(bad))
    return len(bad)


def _env(params, E, N, S):
    from ebcsim.batched import BatchedEnv
    return BatchedEnv(params, E, N, S, device=0)


def _pose_batch(vertices, poses, S):
    """One env per pose, no humans, the scene's polygons in every env; robot = (px, py, 0, 0, radius, 0, 0, 1, theta)."""
    E = len(poses)
    f = lambda *sh: np.zeros(sh)  # noqa: E731
    b = ebc_scene.SceneBatch(E, 1, S, np.zeros(E, np.int32), f(E, 1), f(E, 1), f(E, 1), f(E, 1), f(E, 1), f(E, 1),
                             f(E, 1), f(E, 1), np.zeros((E, 1), np.uint8), np.zeros(E, np.int32), f(E, S), f(E, S),
                             f(E, S), None, f(E, 9))
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 4, 2)
    b.n_poly = np.full(E, len(v), np.int32)
    b.poly = np.zeros((E, S, 4, 2))
    b.poly[:, :len(v)] = v
    for e, (px, py, r, th) in enumerate(poses):
        b.robot[e] = [px, py, 0, 0, r, 0, 0, 1.0, th]
    return b


@pytest.mark.parametrize("fixture", ["local_map", "local_map_edges"])
def test_goldens(fixture, host_lib):
    """ebc_local_map on the golden scenes and poses: the reference's maps bit for bit (the constructed fixture's random
    thetas under the per-pose rule of the CPU tests)."""
    for k, m, pose, want in _fixture_cases(fixture):
        env = _env(_abi.default_params(), len(pose), 1, 20)
        env.configure_local_map(m["dim"], m["max_range"], m["angle_min"], m["angle_max"], m.get("normalize", True))
        env.reset(_pose_batch(m["vertices"], pose, 20))
        g = Guarded((env.E, m["dim"]), torch.float64)
        env.local_map_device(g.t)
        env.synchronize()  # enqueued on the handle's stream
        got = g.check()
        assert _bits_equal(got, env.local_map())
        for i in range(len(pose)):
            if fixture == "local_map":
                assert _bits_equal(got[i], want[i]), (k, i)
            else:
                _check_pose(host_lib, pose[i, 3], got[i], want[i], "%s pose %d" % (m["name"], i))
        env.close()


def _bench_params(kinematics=_abi.HOLONOMIC):
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    p = ebc_config.params_from_config(cfg, pol)
    p.robot_kinematics = kinematics
    return p


def _dims(sc):
    gen = ebc_scene.gen_struct(sc)
    return gen, sum(gen.count), ebc_scene.max_static_rows(sc)


@pytest.mark.parametrize("many", [False, True], ids=["4_walls", "10_circles_10_walls"])
@pytest.mark.parametrize("E", [4096, 4095])
def test_generated_scenes_against_host_build(many, E, host_lib):
    """Device-generated scenes (ebc_generate_reset writes the polygons), random unicycle moves for random positions and
    headings: the step's map and ebc_local_map equal the host build of the same source, bit for bit."""
    sc = _bench_scene_cfg(many)
    gen, N, S = _dims(sc)
    env = _env(_bench_params(_abi.UNICYCLE), E, N, S)
    env.configure_local_map(48, 3.0, -PI, PI)
    env.generate_reset(gen, 5000)
    polys = np.zeros((E, S, 4, 2))
    n_poly = np.zeros(E, np.int32)
    for e in range(E):
        v = np.asarray(ebc_scene.generate_scene(sc, 5000 + e).obstacle_vertices, dtype=np.float64).reshape(-1, 4, 2)
        polys[e, :len(v)], n_poly[e] = v, len(v)
    rs = np.random.RandomState(E)
    robot = env.get_state()["robot"]
    ties = [_assert_device_equals_host(host_lib, env.local_map(), _host_maps(host_lib, polys, n_poly, robot, 48), polys,
                                       n_poly, robot, "reset")]
    for t in range(3):
        act = np.stack([rs.uniform(0, 4.0, E), rs.uniform(-PI, PI, E)], 1)
        out = env.step(act, human_policy=_abi.HUMAN_LINEAR, local_map=True)
        robot = env.get_state()["robot"]
        want = _host_maps(host_lib, polys, n_poly, robot, 48)
        ties.append(_assert_device_equals_host(host_lib, out["local_map"], want, polys, n_poly, robot, "step %d" % t))
        assert _bits_equal(env.local_map(), out["local_map"]), t
    assert (want < 1).any()
    print("envs on atan2 ties per map:", ties)
    env.close()


KEYS = ("reward", "done", "info", "dmin", "dist_to_goal", "robot_action_out", "obs_rotated")


def _auto_reset_run(robot_policy, E=256, P=64, steps=200):
    """Three handles on the same scenes and pool: A steps with maps and auto-reset (device outputs, guarded), B plain
    ebc_step with auto-reset, C with maps and without auto-reset (A's twin up to each env's first terminal step)."""
    import torch
    sc = _bench_scene_cfg(False)
    gen, N, S = _dims(sc)
    envs = [_env(_bench_params(), E, N, S) for _ in range(3)]
    for k, env in enumerate(envs):
        if k != 1:
            env.configure_local_map(48, 3.0, -PI, PI)
        env.generate_reset(gen, 100)
        env.generate_pool(gen, 9000, P)
    A, B, Ctwin = envs
    rs = np.random.RandomState(3)
    first_done = np.full(E, -1)
    g = Guarded((E, 48), torch.float64)
    oa = A.alloc_step_outputs(KEYS)
    oa["local_map"] = g.t
    for t in range(steps):
        act = rs.uniform(-1.0, 1.0, (E, 2)) if robot_policy == _abi.ROBOT_EXTERNAL else None
        ra = None if act is None else torch.from_numpy(act).cuda()
        A.step_device(oa, robot_action=ra, human_policy=_abi.HUMAN_ORCA, robot_policy=robot_policy,
                      flags=_abi.FLAG_AUTO_RESET)
        A.synchronize()
        ma = g.check()
        kw = dict(robot_action=act, human_policy=_abi.HUMAN_ORCA, robot_policy=robot_policy)
        ob = B.step(flags=_abi.FLAG_AUTO_RESET, outputs=KEYS, **kw)
        for k in KEYS:
            assert np.array_equal(oa[k].cpu().numpy().view(np.uint8), ob[k].view(np.uint8)), (k, t)
        oc = Ctwin.step(outputs=("done",), local_map=True, **kw)
        done = oa["done"].cpu().numpy().astype(bool)
        live = first_done < 0
        # up to and including its first terminal step an env's map is its twin's: the terminal state's map
        assert _bits_equal(ma[live], oc["local_map"][live]), t
        first_done[done & live] = t
        cur = A.local_map()
        assert _bits_equal(ma[~done], cur[~done]), t  # non-terminal: the map of the state the env now holds
    assert (first_done >= 0).sum() > E // 4
    for env in envs:
        env.close()


def test_auto_reset_external_actions():
    _auto_reset_run(_abi.ROBOT_EXTERNAL)


def test_auto_reset_linear_robot():
    _auto_reset_run(_abi.ROBOT_LINEAR)


def test_pool_reinstall_keeps_running_polygons():
    """Running envs keep their polygons across pool re-installs: the maps of the current state do not change."""
    sc = _bench_scene_cfg(True)
    gen, N, S = _dims(sc)
    E = 128
    env = _env(_bench_params(), E, N, S)
    env.configure_local_map(48, 3.0, -PI, PI)
    env.generate_reset(gen, 10)
    env.generate_pool(gen, 700, 32)
    for _ in range(60):
        env.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET,
                 outputs=("done",))
    before = env.local_map()
    env.generate_pool(gen, 40000, 16)
    assert _bits_equal(env.local_map(), before)
    scenes = [ebc_scene.generate_scene(sc, 80000 + i) for i in range(8)]
    env.set_scene_pool(ebc_scene.SceneBatch.from_scenes(scenes, N, S))  # a host pool: its polygons are passed on
    assert _bits_equal(env.local_map(), before)
    env.close()


def test_refusals():
    sc = _bench_scene_cfg(False)
    gen, N, S = _dims(sc)
    E = 8
    env = _env(_bench_params(), E, N, S)
    L, h = env._L, env._h
    out = np.zeros((E, 48))
    env.generate_reset(gen, 1)
    assert L.ebc_local_map(h, _abi.HOST, out.ctypes.data) == _abi.ERR_STATE  # before config
    p = _abi.EbcLocalMapParams(struct_size=C.sizeof(_abi.EbcLocalMapParams), dim=129, max_range=3.0, angle_min=-PI,
                               angle_max=PI, normalize=1)
    assert L.ebc_local_map_config(h, C.addressof(p)) == _abi.ERR_UNSUPPORTED  # dim > 128
    env.configure_local_map(48, 3.0, -PI, PI)
    scenes = [ebc_scene.generate_scene(sc, 1 + e) for e in range(E)]
    batch = ebc_scene.SceneBatch.from_scenes(scenes, N, S)
    env.map_dim = 0  # an ebc_reset without ebc_set_obstacles
    env.reset(batch)
    env.map_dim = 48
    assert L.ebc_local_map(h, _abi.HOST, out.ctypes.data) == _abi.ERR_STATE
    assert b"env 0" in L.ebc_last_error()
    env.set_obstacles(batch)
    env.local_map()
    bad = ebc_scene.SceneBatch.from_scenes(scenes, N, S)
    bad.poly[3, 0, 2, 0] += 0.25  # no longer a rectangle
    with pytest.raises(_capi.EbcError) as ei:
        env.set_obstacles(bad)
    assert ei.value.code == _abi.ERR_INVALID
    bad = ebc_scene.SceneBatch.from_scenes(scenes, N, S)
    bad.n_poly[1] = S + 1
    with pytest.raises(_capi.EbcError) as ei:
        env.set_obstacles(bad)
    assert ei.value.code == _abi.ERR_INVALID
    env.map_dim = 0  # a pool without its obstacle pool
    env.set_scene_pool(batch)
    env.map_dim = 48
    assert L.ebc_local_map(h, _abi.HOST, out.ctypes.data) == _abi.ERR_STATE
    assert b"pool scene 0" in L.ebc_last_error()
    args = _abi.EbcStepArgs(struct_size=C.sizeof(_abi.EbcStepArgs), location=_abi.HOST, human_policy=_abi.HUMAN_ORCA,
                            robot_policy=_abi.ROBOT_LINEAR)
    assert L.ebc_step_with_map(h, C.addressof(args), out.ctypes.data) == _abi.ERR_STATE
    env.set_obstacle_pool(batch)
    assert L.ebc_step_with_map(h, C.addressof(args), out.ctypes.data) == 0
    env.close()


def test_facade_device_map_on_wall_episode(host_lib):
    """The facade on the device, a golden wall scene: every map equals get_local_map_angular of the robot's state
    (bit for bit where sincos_dd and numpy agree on theta), and map calls are not backend calls."""
    from ebcsim import env as ebc_env
    from ebcsim.agents import Robot
    from ebcsim.policy import policy_factory
    row = _static_known_answer()
    cfg = configparser.RawConfigParser()
    cfg.read_string(row["config_text"])
    env = ebc_env.make()
    env.configure(cfg)
    robot = Robot(cfg, "robot")
    env.set_robot(robot)
    robot.set_policy(policy_factory["linear"]())
    ob, local_map = env.reset("test", load_scene_path=os.path.join(GOLDEN, "scenes", row["scene"]))
    assert env._device_map

    poly = np.asarray(env.scene.obstacle_vertices, dtype=np.float64)

    def check(m, what):
        want = env.get_local_map_angular(robot.get_full_state(), append=False)
        if not _bits_equal(m, want):  # only where a sector quotient sits on an integer (_atan2_tie)
            assert _atan2_tie(host_lib, poly, [robot.px, robot.py, robot.radius, robot.theta]), what
            return
        _check_pose(host_lib, robot.theta, m, want, what)
    check(local_map, "reset")
    done, steps = False, 0
    while not done:
        action = robot.act(ob, local_map=local_map, env=env)
        check(env.step(action, update=False)[1], "look-ahead %d" % steps)
        ob, local_map, reward, done, info = env.step(action)
        steps += 1
        check(local_map, "step %d" % steps)
        assert steps < 500
    assert env.backend_calls == 2 * steps
    assert len(env.local_maps_angular) == 1 + 2 * steps
