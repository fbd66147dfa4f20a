#!/usr/bin/env python3
"""Device time of a CADRL decision batch: `--envs` envs x 81 actions on the bench workload's scenes (10 humans + 8 static
rows), with its parts (the look-ahead sweep, the value network's two float32 blocks on every row, the decision kernel
ebc_cadrl_decide alone) and the SARL decision on the same box beside it.

    python3 tools/cadrl_bench.py [--envs 1024] [--blocks 7] [--reps 5] [--out profiles/cadrl_decision.txt]

Warm-up first, then the median over `--blocks` blocks of `--reps` back-to-back calls, each block timed with a pair of
events on the stream (device time; a decision's host side overlaps the kernels of the one before)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0] + " (policies: cadrl, sarl)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    import bench
    from ebcsim import _abi, actions as ebc_actions
    from ebcsim.batched import BatchedEnv
    from ebcsim.cadrl import CadrlModule, CadrlValueNet, DeviceCadrlPolicy, native_decide
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
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

    E = args.envs
    gold = os.path.join(ROOT, "tests", "golden", "weights")
    say("# tools/cadrl_bench.py --envs %d --blocks %d --reps %d: device ms per call, median (min .. max) of the blocks; %s"
        % (E, args.blocks, args.reps, torch.cuda.get_device_name(0)))

    def cadrl_net():
        """An untrained network of the shape every policy config of the reference gives (times do not depend on the values)."""
        torch.manual_seed(11)
        return CadrlValueNet(CadrlModule(13, [150, 100, 100, 1]).state_dict(), device="cuda:0")
    for typed, label in ((0, "cadrl"), (1, "sarl (shipped eb-cadrl weights)")):
        params, batch = bench.build_batch("metric", E, 0)
        params.with_agent_type = typed
        env = BatchedEnv(params, E, batch.N, batch.S)
        env.reset(batch)
        env.use_torch_stream()
        space = ebc_actions.build_action_space(float(batch.robot[0, 7]))
        if typed:
            pol = DeviceSarlPolicy(SarlValueNet.load(os.path.join(gold, "sarl_n10_ebcadrl.pth"), device="cuda:0"), space, 0.9)
        else:
            net = cadrl_net()
            pol = DeviceCadrlPolicy(net, space, 0.9)
        med, lo, hi = timed(lambda: pol.decide(env))
        say("decision  %-36s E %d x A %d x R %d: %8.3f ms (%.3f .. %.3f)" % (label, E, len(space), env.R, med, lo, hi))
        med, lo, hi = timed(lambda: env.lookahead_device(pol._acts, pol._bufs, human_policy=_abi.HUMAN_ORCA))
        say("  of which the look-ahead sweep alone:                              %8.3f ms (%.3f .. %.3f)" % (med, lo, hi))
        if not typed:
            rows, reward = pol._bufs["rows_rotated"], pol._bufs["reward"]
            A = rows.shape[1]
            x = rows.view(-1, env.T)
            blocks = net._native_blocks()
            med, lo, hi = timed(lambda: blocks[1].f32(blocks[0].f32(x, True), False))
            say("  the value network, two float32 blocks on %d rows:            %8.3f ms (%.3f .. %.3f)" % (x.shape[0], med, lo, hi))
            v = blocks[1].f32(blocks[0].f32(x, True), False).view(E, A, env.R)
            values = torch.empty((E, A), dtype=torch.float64, device="cuda:0")
            choice = torch.empty((E,), dtype=torch.int32, device="cuda:0")
            med, lo, hi = timed(lambda: native_decide(v, reward, 0.9, None, values, choice))
            say("  the decision kernel alone (min over %d rows, value, choice):     %8.3f ms (%.3f .. %.3f)" % (env.R, med, lo, hi))
        env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
