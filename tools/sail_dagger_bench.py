#!/usr/bin/env python3
"""Per-step time of a DAgger window (the SAIL network drives, the ORCA robot labels every state, a mask at beta 0.5 says
whose action a step executes) on device-generated scenes, `--envs` envs x `--adults` adults, `--steps` steps, from the
same reset:

    (a) ONE ebc_sail_dagger_k call: per step the label kernel, the network, the select, the step (four launches)
    (b) the Python composition of the entries that were there before it, seven enqueues per step: robot_state_device,
        observe_ob_device, row_counts_device, ebc_sail_forward on those, robot_orca_device, torch.where on the mask,
        step_device
    (c) ebc_step_k with EBC_ROBOT_SAIL, the closed loop without an expert, for scale

    python3 tools/sail_dagger_bench.py [--envs 4096,1024] [--adults 5] [--steps 40] [--blocks 9] [--out profiles/sail_dagger.txt]

Every form is timed as wall time from a synchronised start to a synchronised end of the whole window (what a caller waits
for; (b) is bound by its host side, which device events would hide) and with a pair of events on the stream.  Two warm-up
windows per form, then `--blocks` blocks in which the forms alternate; median and min .. max of the per-step time, and the
spread (max - min) that a difference between two forms has to exceed.  The records and actions of (a) and (b) are compared at the end: the same
bytes."""
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
    ap = argparse.ArgumentParser(description="DAgger window per step: ebc_sail_dagger_k, the seven-call Python loop, ebc_step_k with EBC_ROBOT_SAIL")
    ap.add_argument("--envs", default="4096,1024", help="comma-separated env counts")
    ap.add_argument("--adults", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=9, help="timed blocks (one window of every form each), after two warm-up windows per form")
    ap.add_argument("--forms", default="abc")
    ap.add_argument("--safety-space", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _abi, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailModule, SailNet, native_forward
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    N, K = args.adults, args.steps
    say("# tools/sail_dagger_bench.py --envs %s --adults %d --steps %d --blocks %d: us per step, median (min .. max) of the "
        "windows; %s" % (args.envs, N, K, args.blocks, torch.cuda.get_device_name(0)))
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol, policy="sail")
    sc = ebc_scene.SceneConfig.from_config(cfg)
    sc.adult_num, sc.bicycle_num, sc.children_num, sc.num_circles, sc.num_walls = N, 0, 0, 0, 0
    gen = ebc_scene.gen_struct(sc, "test")
    torch.manual_seed(11)  # an untrained network (times do not depend on the values)
    net = SailNet(SailModule(N).state_dict(), device="cuda:0")
    AUTO = _abi.FLAG_AUTO_RESET
    for E in [int(x) for x in args.envs.split(",")]:
        env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
        env.use_torch_stream()
        env.attach_sail(net)
        policy = DeviceSailPolicy(net)
        take = torch.rand((K, E), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(5)) < 0.5
        out_a, out_b = env.alloc_sail_dagger_outputs(K), env.alloc_sail_dagger_outputs(K)
        out_c = env.alloc_step_k_outputs(K, ("robot_action_out", "reward", "done", "info"))
        step_b = [{k: out_b[k][t] for k in ("reward", "done", "info")} for t in range(K)]
        nat = net.native()

        def entry():
            env.sail_dagger_k_device(out_a, K, take_expert=take, safety_space=args.safety_space, flags=AUTO)

        def python_loop():
            o = out_b
            for t in range(K):
                env.robot_state_device(o["robot"][t])
                env.observe_ob_device(o["ob"][t])
                env.row_counts_device(o["n_rows"][t])
                native_forward(nat._h, o["robot"][t], o["ob"][t], o["n_rows"][t], o["learner_action"][t], want_feat=False)
                env.robot_orca_device(o["expert_action"][t], args.safety_space)
                torch.where(take[t][:, None], o["expert_action"][t], o["learner_action"][t], out=o["robot_action_out"][t])
                env.step_device(step_b[t], robot_action=o["robot_action_out"][t], human_policy=_abi.HUMAN_ORCA, flags=AUTO)

        forms = {"a": ("(a) ebc_sail_dagger_k, 4 launches per step", entry),
                 "b": ("(b) Python loop of 7 enqueues per step", python_loop),
                 "c": ("(c) ebc_step_k, EBC_ROBOT_SAIL (no expert)", lambda: policy.rollout(env, K, out_c, flags=AUTO))}
        say("## %d envs x %d adults, %d steps per window" % (E, N, K))
        def window(fn):
            env.generate_reset(gen, 1000)  # every window runs the same K steps
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / K * 1e6, e0.elapsed_time(e1) / K * 1e3

        for f in args.forms:  # warm-up: code objects, allocations, the argument caches
            for _ in range(2):
                window(forms[f][1])
        wall, dev = {f: [] for f in args.forms}, {f: [] for f in args.forms}
        for _ in range(args.blocks):  # the forms alternate, so a drift of the machine meets all of them
            for f in args.forms:
                w, d = window(forms[f][1])
                wall[f].append(w)
                dev[f].append(d)
        med, spread = {}, {}
        for f in args.forms:
            med[f], spread[f] = statistics.median(wall[f]), max(wall[f]) - min(wall[f])
            say("%-46s wall %8.2f us (%.2f .. %.2f, spread %.2f)   stream events %8.2f us (%.2f .. %.2f)" % (
                forms[f][0], med[f], min(wall[f]), max(wall[f]), spread[f], statistics.median(dev[f]), min(dev[f]), max(dev[f])))
        if "a" in med and "b" in med:
            say("(b) / (a): %.2f x; (b) - (a) = %.2f us per step against (b)'s spread of %.2f us" % (
                med["b"] / med["a"], med["b"] - med["a"], spread["b"]))
            same = all(bool((out_a[k].reshape(-1).view(torch.uint8) == out_b[k].reshape(-1).view(torch.uint8)).all()) for k in out_a)
            say("records, actions and step outputs of (a) and (b): %s; executed actions finite: %s" % (
                "the same bytes" if same else "DIFFERENT", bool(torch.isfinite(out_a["robot_action_out"]).all())))
        if "a" in med and "c" in med:
            say("(a) / (c): %.2f x (the price of the labels)" % (med["a"] / med["c"]))
        env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
