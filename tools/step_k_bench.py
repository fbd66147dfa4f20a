#!/usr/bin/env python3
"""Per-step time of ebc_step_k with and without EBC_FLAG_ONE_LAUNCH (the K steps as one kernel launch):

    python3 tools/step_k_bench.py [--envs 4096 16384] [--K 50] [--repeats 5] [--robots orca linear external] [--outputs a b]

The metric config (eb-cadrl_amd/configs/bench_metric.config: 10 humans, 4 walls) on device-generated scenes, ORCA
humans, auto-reset from a generated pool, for the three robot policies, with (a) state_rotated + reward / done / info
(what train.collect_il asks for) and (b) reward / done / info only.  Both forms run in the same process from the same
reset and the same freshly installed pool; HIP events around the whole call; `repeats` timed calls after two warm-up calls; median and min-max of the
per-step time, one JSON line per case.  Kernels per call:
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/step_k_bench.py --envs 4096 --repeats 1 --robots orca --outputs a
Traffic per step (counter runs of their own, no tracing beside them; FETCH_SIZE and WRITE_SIZE in separate passes):
    rocprofv3 --pmc FETCH_SIZE -d out -- python3 tools/step_k_bench.py --envs 4096 --repeats 1 --robots orca --outputs a"""
import argparse
import configparser
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--robots", nargs="+", default=["orca", "linear", "external"])
    ap.add_argument("--outputs", nargs="+", default=["a", "b"], choices=["a", "b"],
                    help="a: state_rotated + reward / done / info; b: reward / done / info")
    args = ap.parse_args()
    import numpy as np
    import torch
    from ebcsim import _abi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv

    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "test")
    N, S = sum(gen.count), ebc_scene.max_static_rows(sc)
    K = args.K
    for E in args.envs:
        env = BatchedEnv(params, E, N, S)
        env.use_torch_stream()
        env.generate_reset(gen, 1000)
        env.generate_pool(gen, 100000, E)
        v_pref = float(env.get_state()["robot"][0, 7])
        space = ebc_actions.build_action_space(v_pref)
        rs = np.random.RandomState(3)
        ext = torch.tensor(space[rs.randint(len(space), size=(K, E))], dtype=torch.float64, device="cuda")
        for robot in args.robots:
            kw = dict(human_policy=_abi.HUMAN_ORCA)
            if robot == "orca":
                kw.update(robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)
            elif robot == "linear":
                kw.update(robot_policy=_abi.ROBOT_LINEAR)
            else:
                kw.update(robot_policy=_abi.ROBOT_EXTERNAL, robot_action=ext)
            for case, label, keys in (("a", "state_rotated+reward+done+info", ("state_rotated", "reward", "done", "info")),
                                      ("b", "reward+done+info", ("reward", "done", "info"))):
                if case not in args.outputs:
                    continue
                outs = env.alloc_step_k_outputs(K, keys)
                res = {}
                for form, extra in (("per_step", 0), ("one_launch", _abi.FLAG_ONE_LAUNCH)):
                    # both forms time the same K steps: the same start scenes, and the pool installed again so that
                    # every env's cursor is back at its first restart scene
                    env.generate_reset(gen, 1000)
                    env.generate_pool(gen, 100000, E)
                    fl = _abi.FLAG_AUTO_RESET | extra
                    times = []
                    for it in range(2 + args.repeats):
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        env.step_k_device(outs, K, flags=fl, **kw)
                        e1.record()
                        torch.cuda.synchronize()
                        if it >= 2:
                            times.append(e0.elapsed_time(e1) / K * 1e3)  # us per step
                    env.synchronize()
                    res[form] = dict(median_us=round(statistics.median(times), 2), min_us=round(min(times), 2),
                                     max_us=round(max(times), 2))
                print(json.dumps(dict(envs=E, humans=N, static_rows=S, K=K, robot=robot, outputs=label, repeats=args.repeats,
                                      **{f + "_" + k: v for f, r in res.items() for k, v in r.items()},
                                      speedup=round(res["per_step"]["median_us"] / res["one_launch"]["median_us"], 3))),
                      flush=True)
        env.close()


if __name__ == "__main__":
    main()
