#!/usr/bin/env python3
"""Device time of a SAIL decision batch on device-generated scenes: `--envs` envs x `--adults` adults (the bench
workload's env config with that many adults and nothing else), three ways on the same inputs — the kernel alone
(ebc_sail_forward), DeviceSailPolicy.decide (the robot state, the observation and the row counts from the handle, then
the kernel) and the torch module SailModule on the same device (the yard-stick: about 20 launches per decision).

    python3 tools/sail_bench.py [--envs 4096] [--adults 5] [--blocks 7] [--reps 5] [--out profiles/sail_decision.txt]

Warm-up first, then the median over `--blocks` blocks of `--reps` back-to-back calls, each block timed with a pair of
events on the stream (device time; a call's host side overlaps the kernels of the one before)."""
import argparse
import configparser
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0] + " (policy: sail)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--adults", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailModule, SailNet, native_forward
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.reps)
        return statistics.median(ms), min(ms), max(ms)

    E, N = args.envs, args.adults
    say("# tools/sail_bench.py --envs %d --adults %d --blocks %d --reps %d: device ms per call, median (min .. max) of the "
        "blocks; %s" % (E, N, args.blocks, args.reps, torch.cuda.get_device_name(0)))
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol, policy="sail")
    sc = ebc_scene.SceneConfig.from_config(cfg)
    sc.adult_num, sc.bicycle_num, sc.children_num, sc.num_circles, sc.num_walls = N, 0, 0, 0, 0
    gen = ebc_scene.gen_struct(sc, "test")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    env.generate_reset(gen, 1000)
    # an untrained network of the only shape SAIL.configure builds (times do not depend on the values)
    torch.manual_seed(11)
    net = SailNet(SailModule(N).state_dict(), device="cuda:0")
    policy = DeviceSailPolicy(net)
    actions, _ = policy.decide(env)
    torch.cuda.synchronize()
    b = policy._bufs
    assert int((b["n_rows"] != N).sum()) == 0 and bool(torch.isfinite(actions).all()), "the generated scenes do not have %d rows each" % N
    med, lo, hi = timed(lambda: native_forward(net.native()._h, b["robot"], b["ob"], b["n_rows"], b["action"], b["feat_joint"]))
    say("the kernel alone (ebc_sail_forward)              E %d x N %d: %8.3f ms (%.3f .. %.3f)" % (E, N, med, lo, hi))
    kernel_ms = med
    med, lo, hi = timed(lambda: policy.decide(env))
    say("DeviceSailPolicy.decide (state, rows, counts, kernel)        : %8.3f ms (%.3f .. %.3f)" % (med, lo, hi))
    robot32 = b["robot"][:, [0, 1, 2, 3, 5, 6]].to(torch.float32).contiguous()
    crowd32 = b["ob"][:, :N, :4].to(torch.float32).contiguous()
    with torch.no_grad():
        want = net.module(robot32, crowd32)[0]
        med, lo, hi = timed(lambda: net.module(robot32, crowd32))
    say("SailModule in torch on the same device, same inputs (cast)   : %8.3f ms (%.3f .. %.3f)" % (med, lo, hi))
    say("torch / kernel: %.2f x; largest |kernel - torch| over the batch's actions: %.3g" % (
        med / kernel_ms, float((b["action"] - want.double()).abs().max())))
    env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
