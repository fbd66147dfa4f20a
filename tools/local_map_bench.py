#!/usr/bin/env python3
"""Time the angular local map (get_local_map_angular, simulator/env.py:468-628) on device-generated scenes:

    python3 tools/local_map_bench.py [--envs 4096 16384] [--steps 50]

Per (obstacle config, E): ebc_local_map alone, ebc_step, and ebc_step_with_map (the step plus the map of its post-step
state), each the mean of `steps` back-to-back calls between two HIP events; then the host restatement
(ebcsim/local_map.py) per env, for scale.  Obstacle configs: eb-cadrl_amd/configs/bench_metric.config (the headline
workload: 10 humans, 4 walls) and the same with num_circles = num_walls = 10 (20 polygons).  Map parameters, passed
explicitly: dim 48, range 3, angles +-pi (the shipped reference configs' values; bench_metric.config has no angular-map
keys).  Humans: ORCA; robot: the linear policy; auto-reset from a generated pool.  Device time per kernel:
rocprofv3 --kernel-trace --stats -d out -- python3 tools/local_map_bench.py"""
import argparse
import configparser
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)

DIM, RANGE = 48, 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--host-envs", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    from ebcsim import _abi, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.local_map import angular_map

    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol)
    for name, extra in (("4_walls", None), ("10_circles_10_walls", (10, 10))):
        sc = ebc_scene.SceneConfig.from_config(cfg)
        if extra:
            sc.num_circles, sc.num_walls = extra
        gen = ebc_scene.gen_struct(sc, "test")
        N, S = sum(gen.count), ebc_scene.max_static_rows(sc)
        for E in args.envs:
            env = BatchedEnv(params, E, N, S)
            env.use_torch_stream()
            env.configure_local_map(DIM, RANGE, -np.pi, np.pi)
            env.generate_reset(gen, 1000)
            env.generate_pool(gen, 100000, E)
            m = torch.zeros((E, DIM), dtype=torch.float64, device="cuda")
            plain = env.alloc_step_outputs(("reward", "done", "info", "obs_rotated"))
            withmap = dict(plain, local_map=m)
            kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET)

            def timed(fn):
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / args.steps * 1e3  # us per call
            t_map = timed(lambda: env.local_map_device(m))
            t_step = timed(lambda: env.step_device(plain, **kw))
            t_both = timed(lambda: env.step_device(withmap, **kw))
            env.synchronize()
            print(json.dumps(dict(config=name, envs=E, polygons=sc.num_circles + sc.num_walls,
                                  local_map_us=round(t_map, 2), step_us=round(t_step, 2),
                                  step_with_map_us=round(t_both, 2), map_ns_per_env=round(t_map * 1e3 / E, 2))),
                  flush=True)
            env.close()
        scenes = [ebc_scene.generate_scene(sc, 1000 + i) for i in range(args.host_envs)]
        t0 = time.perf_counter()
        for s in scenes:
            r = s.robot
            angular_map(s.obstacle_vertices, r[0], r[1], r[4], r[8], RANGE, DIM, -np.pi, np.pi)
        host_us = (time.perf_counter() - t0) / len(scenes) * 1e6
        print(json.dumps(dict(config=name, host_restatement_us_per_env=round(host_us, 1))), flush=True)


if __name__ == "__main__":
    main()
