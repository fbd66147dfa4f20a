#!/usr/bin/env python3
"""Per-step time of a SAIL closed loop on device-generated scenes, `--envs` envs x `--adults` adults (the bench
workload's env config with that many adults and nothing else), `--steps` steps, three ways from the same reset:

    (a) the Python loop: DeviceSailPolicy.decide + BatchedEnv.step_device per step (five launches and the host between)
    (b) the per-step form: ONE ebc_step_k call with EBC_ROBOT_SAIL (the same launches, no host work between them)
    (c) the one-launch form: the same call with EBC_FLAG_ONE_LAUNCH (the network inside the rollout kernel)

    python3 tools/sail_rollout_bench.py [--envs 4096] [--adults 5] [--steps 40] [--repeats 7] [--out profiles/sail_rollout.txt]

Every form is timed as wall time from a synchronised start to a synchronised end of the whole `--steps`-step window
(what a caller waits for: (a) is bound by its host side, which device events around the kernels would hide) and, for (b)
and (c), with a pair of events on the stream as well.  Two warm-up windows, then `--repeats` windows; median and min ..
max of the per-step time.  The actions of the three forms are compared at the end: they are the same bytes.  Kernels of
the one-launch form, in a run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/sail_rollout_bench.py --repeats 1 --forms c"""
import argparse
import configparser
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description="SAIL closed loop per step: Python loop, per-step ebc_step_k, one-launch ebc_step_k")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--adults", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--forms", default="abc", help="which of a (Python loop), b (per-step), c (one-launch) to run")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _abi, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailModule, SailNet
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    E, N, K = args.envs, args.adults, args.steps
    say("# tools/sail_rollout_bench.py --envs %d --adults %d --steps %d --repeats %d: us per step, median (min .. max) of the "
        "windows; %s" % (E, N, K, args.repeats, torch.cuda.get_device_name(0)))
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol, policy="sail")
    sc = ebc_scene.SceneConfig.from_config(cfg)
    sc.adult_num, sc.bicycle_num, sc.children_num, sc.num_circles, sc.num_walls = N, 0, 0, 0, 0
    gen = ebc_scene.gen_struct(sc, "test")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    torch.manual_seed(11)  # an untrained network of the only shape SAIL.configure builds (times do not depend on the values)
    policy = DeviceSailPolicy(SailNet(SailModule(N).state_dict(), device="cuda:0"))
    keys = ("robot_action_out", "reward", "done", "info")
    outs = env.alloc_step_k_outputs(K, keys)
    step_outs = [{k: outs[k][t] for k in keys} for t in range(K)]

    def python_loop():
        for t in range(K):
            actions, _ = policy.decide(env)
            env.step_device(step_outs[t], robot_action=actions, human_policy=_abi.HUMAN_ORCA, flags=_abi.FLAG_AUTO_RESET)

    forms = {"a": ("(a) Python loop: decide + step_device per step", python_loop),
             "b": ("(b) per-step form: ebc_step_k, EBC_ROBOT_SAIL", lambda: policy.rollout(env, K, outs, flags=_abi.FLAG_AUTO_RESET)),
             "c": ("(c) one-launch form: + EBC_FLAG_ONE_LAUNCH", lambda: policy.rollout(env, K, outs, flags=_abi.FLAG_AUTO_RESET | _abi.FLAG_ONE_LAUNCH))}
    medians, actions = {}, {}
    for f in args.forms:
        label, fn = forms[f]
        wall, dev = [], []
        for it in range(2 + args.repeats):
            env.generate_reset(gen, 1000)  # every window runs the same K steps
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= 2:
                wall.append((t1 - t0) / K * 1e6)
                dev.append(e0.elapsed_time(e1) / K * 1e3)
        actions[f] = outs["robot_action_out"].clone()
        medians[f] = statistics.median(wall)
        say("%-52s wall %8.2f us (%.2f .. %.2f)   stream events %8.2f us (%.2f .. %.2f)" % (
            label, medians[f], min(wall), max(wall), statistics.median(dev), min(dev), max(dev)))
    if "a" in medians:
        for f in "bc":
            if f in medians:
                say("(a) / (%s): %.2f x" % (f, medians["a"] / medians[f]))
    if "b" in medians and "c" in medians:
        say("(b) / (c): %.2f x" % (medians["b"] / medians["c"]))
    first = actions[args.forms[0]]
    same = all(bool((a.view(torch.int64) == first.view(torch.int64)).all()) for a in actions.values())
    say("robot_action_out of the forms run: %s; finite: %s" % ("the same bytes" if same else "DIFFERENT",
                                                                 bool(torch.isfinite(first).all())))
    env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
