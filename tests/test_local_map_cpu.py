"""The angular local map (get_local_map_angular, simulator/env.py:468-628) without a GPU.

The source the kernel compiles (eb-cadrl_amd/csrc/ebc_local_map.h) built for the host with g++
(tests/native/local_map_host.cc) against the reference's own outputs (tests/golden/local_map.npz: 9 scenes x 12 poses;
tests/golden/local_map_edges.npz: constructed corner cases, tests/golden/make_local_map_edges.py) and against
ebcsim/local_map.py on random scenes.  cos / sin of theta come from sincos_dd, numpy's from a CPU-dependent routine:
where the two agree the maps must agree bit for bit; elsewhere (about 1 pose in 700) within a few ulps per sector,
with the same sectors left at max_range.  Also: the generator's polygons (ebc_scene_gen.h) against scene.py, the new
ABI structs against the header, and the facade on a backend without a device map."""
import configparser
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from ebcsim import _abi, scene as ebc_scene
from ebcsim.local_map import angular_map
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")


def _build(tmp_path_factory, name, src):
    so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", src), "-o", so], check=True, timeout=300)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def host_map(tmp_path_factory):
    lib = _build(tmp_path_factory, "local_map_host", "local_map_host.cc")

    def run(vertices, poses, dim, max_range, angle_min, angle_max, normalize=True):
        poly = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 4, 2))
        pose = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
        out = np.zeros((len(pose), dim))
        lib.local_map_host(C.c_void_p(poly.ctypes.data), len(poly), C.c_void_p(pose.ctypes.data), len(pose), int(dim),
                           C.c_double(max_range), C.c_double(angle_min), C.c_double(angle_max), int(bool(normalize)),
                           C.c_void_p(out.ctypes.data))
        return out

    run.lib = lib
    return run


def _sincos_agrees(lib, theta):
    c, s = C.c_double(), C.c_double()
    lib.sincos_dd_host(C.c_double(theta), C.byref(c), C.byref(s))
    return c.value == np.cos(theta) and s.value == np.sin(theta)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _fixture_cases(name):
    z = load(name)
    for k in range(int(z["n"])):
        m = json.loads(str(z["meta_%d" % k]))
        yield k, m, z["pose_%d" % k], z["map_%d" % k]


def test_host_build_equals_reference_goldens(host_map):
    """All 9 scenes x 12 poses of the reference's own maps, bit for bit (every golden theta agrees with numpy's)."""
    for k, m, pose, want in _fixture_cases("local_map"):
        got = host_map(m["vertices"], pose, m["dim"], m["max_range"], m["angle_min"], m["angle_max"])
        assert _bits_equal(got, want), "scene %d" % k


def _check_pose(lib, theta, got, want, what):
    if _sincos_agrees(lib, theta):
        assert _bits_equal(got, want), what
    else:  # cos / sin an ulp apart: distances may move in their last bits, no sector changes
        np.testing.assert_array_equal(got == got.max(), want == want.max(), err_msg=what)
        np.testing.assert_allclose(got, want, rtol=4 * np.finfo(float).eps, atol=0, err_msg=what)


def test_host_build_equals_reference_edge_cases(host_map):
    """Constructed by the reference itself: ry = +0 at theta = 0 (sector dim), polygons across the +-pi cut
    (wrapped spans dropped past dim), spans of exactly dim / 2, the robot's box inside an obstacle, dim = 72 and
    normalize = False."""
    names = set()
    for k, m, pose, want in _fixture_cases("local_map_edges"):
        names.add(m["name"])
        got = host_map(m["vertices"], pose, m["dim"], m["max_range"], m["angle_min"], m["angle_max"], m["normalize"])
        for i in range(len(pose)):
            _check_pose(host_map.lib, pose[i, 3], got[i], want[i], "%s pose %d" % (m["name"], i))
        if m["name"] != "raw":
            assert (want <= 1).all()
    assert names == {"level_corner", "pi_cut", "half_span", "overlap", "dim72", "raw"}


def test_edge_fixture_reaches_its_corners():
    """The constructed poses do reach what they are named for (checked with the Python restatement's arithmetic)."""
    z = {m["name"]: (m, pose) for _, m, pose, _ in _fixture_cases("local_map_edges")}
    m, pose = z["level_corner"]
    res = (m["angle_max"] - m["angle_min"]) / m["dim"]
    hits = set()
    for px, py, r, th in pose:
        for v in np.asarray(m["vertices"]).reshape(-1, 2):
            for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
                ry = (v[1] - (py + sy * r)) * np.cos(th) - (v[0] - (px + sx * r)) * np.sin(th)
                rx = (v[0] - (px + sx * r)) * np.cos(th) + (v[1] - (py + sy * r)) * np.sin(th)
                if ry == 0 and rx < 0:
                    hits.add(int((math.atan2(ry, rx) - m["angle_min"]) / res))
    assert m["dim"] in hits  # atan2(+0, x < 0) = +pi: a sector that is never stored but takes part in walks
    assert len(z["half_span"][1]) >= 4 and z["dim72"][0]["dim"] == 72 and z["raw"][0]["normalize"] is False


def _random_scene(rs):
    polys = []
    for _ in range(rs.randint(1, 21)):
        xm, ym = rs.uniform(-4, 4), rs.uniform(-4, 4)
        hx, hy = (rs.uniform(0.1, 1.0), rs.uniform(0.1, 1.0)) if rs.rand() < 0.5 else (rs.randint(1, 5) / 2.0, 0.5)
        polys.append([[xm + hx, ym + hy], [xm - hx, ym + hy], [xm - hx, ym - hy], [xm + hx, ym - hy]])
    return polys


def test_host_build_equals_restatement_random(host_map):
    """200 seeded random scenes / poses against ebcsim/local_map.py, under the per-pose rule."""
    rs = np.random.RandomState(5)
    disagree = 0
    for t in range(200):
        polys = _random_scene(rs)
        pose = [rs.uniform(-4, 4), rs.uniform(-4, 4), [0.2, 0.3][t % 2], rs.uniform(-np.pi, np.pi)]
        dim = [48, 72][t % 2]
        want = angular_map(polys, *pose, 3.0, dim, -np.pi, np.pi)
        got = host_map(polys, [pose], dim, 3.0, -np.pi, np.pi)[0]
        _check_pose(host_map.lib, pose[3], got, want, "random case %d" % t)
        disagree += not _sincos_agrees(host_map.lib, pose[3])
    assert disagree < 10


BENCH_CFG = os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config")


def _bench_scene_cfg(many):
    cfg = configparser.RawConfigParser()
    cfg.read(BENCH_CFG)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    if many:  # the bench tool's second obstacle config: 10 circles + 10 walls
        sc.num_circles, sc.num_walls = 10, 10
    return sc


@pytest.mark.parametrize("many", [False, True], ids=["4_walls", "10_circles_10_walls"])
def test_generated_polygons_equal_scene_py(host_map, many):
    """The generator's polygons (ebc_scene_gen.h, host build) are scene.py's obstacle_vertices for 500 seeds."""
    sc = _bench_scene_cfg(many)
    gen = ebc_scene.gen_struct(sc)
    seeds = np.arange(3000, 3500, dtype=np.uint32)
    N = sum(gen.count)
    S = ebc_scene.max_static_rows(sc)
    G = int(round(sc.map_size_m / sc.map_resolution))
    poly = np.zeros((len(seeds), S, 4, 2))
    n_poly = np.zeros(len(seeds), np.int32)
    rc = host_map.lib.scene_gen_poly_host(C.byref(gen), C.c_void_p(seeds.ctypes.data), len(seeds), N, S, G,
                                          C.c_void_p(poly.ctypes.data), C.c_void_p(n_poly.ctypes.data))
    assert rc == 0
    for r, seed in enumerate(seeds):
        want = np.asarray(ebc_scene.generate_scene(sc, int(seed)).obstacle_vertices, dtype=np.float64).reshape(-1, 4, 2)
        assert n_poly[r] == len(want) == sc.num_circles + sc.num_walls
        assert _bits_equal(poly[r, :n_poly[r]], want), "seed %d" % seed
        assert not poly[r, n_poly[r]:].any()


def test_local_map_struct_sizes_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n",'
                   'sizeof(EbcLocalMapParams),sizeof(EbcObstacles),offsetof(EbcLocalMapParams,normalize),'
                   'offsetof(EbcObstacles,vertices));return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert sizes == [C.sizeof(_abi.EbcLocalMapParams), C.sizeof(_abi.EbcObstacles),
                     _abi.EbcLocalMapParams.normalize.offset, _abi.EbcObstacles.vertices.offset]


def test_scene_batch_carries_polygons():
    sc = _bench_scene_cfg(True)
    scenes = [ebc_scene.generate_scene(sc, s) for s in (11, 12)]
    b = ebc_scene.SceneBatch.from_scenes(scenes)
    assert b.poly.shape == (2, b.S, 4, 2) and list(b.n_poly) == [20, 20]
    np.testing.assert_array_equal(b.poly[1, :20], np.asarray(scenes[1].obstacle_vertices))


def _static_known_answer():
    with open(os.path.join(ROOT, "tests", "golden", "known_answers.json")) as f:
        return next(r for r in json.load(f) if r["scene"] == "collision_with_static.json")


def test_facade_on_oracle_backend_keeps_host_map():
    """A backend without local_map (the CPU oracle): reset / step maps are ebcsim/local_map.py's."""
    from oracle import oracle
    from ebcsim import env as ebc_env
    from ebcsim.action import ActionXY
    from ebcsim.agents import Robot
    from ebcsim.policy import policy_factory
    row = _static_known_answer()
    cfg = configparser.RawConfigParser()
    cfg.read_string(row["config_text"])
    env = ebc_env.make(backend_factory=lambda p, E, N, S: oracle.OracleEnv(p, E, N, S))
    env.configure(cfg)
    robot = Robot(cfg, "robot")
    env.set_robot(robot)
    robot.set_policy(policy_factory["linear"]())
    ob, local_map = env.reset("test", load_scene_path=os.path.join(ROOT, "tests", "golden", "scenes", row["scene"]))
    assert env._device_map is False and len(env.scene.obstacle_vertices) > 0
    want = angular_map(env.scene.obstacle_vertices, robot.px, robot.py, robot.radius, robot.theta,
                       env.angular_map_max_range, env.angular_map_dim, env.angular_map_min_angle,
                       env.angular_map_max_angle)
    assert _bits_equal(local_map, want)
    ob, local_map, reward, done, info = env.step(ActionXY(0.3, 0.4))
    want = env.get_local_map_angular(robot.get_full_state(), append=False)
    assert _bits_equal(local_map, want) and len(env.local_maps_angular) == 2
    assert env.backend_calls == 1
