#!/usr/bin/env python3
"""Device time of the occupancy-map kernel (ebc_occupancy_rows) alone and of a SARL decision batch with and without maps:
`--envs` envs x 81 actions on the bench workload's scenes (10 humans + 8 static rows, rows 17 wide; the maps of the shipped
[om] section, 4 x 4 cells x 3 channels, make them 65 wide).

    python3 tools/om_bench.py [--envs 1024] [--blocks 7] [--reps 5] [--out profiles/om_decision.txt]

Warm-up first, then the median over `--blocks` blocks of `--reps` back-to-back calls, each block timed with a pair of
events on the stream (device time).  The kernel's rate counts the bytes it must move: rows read once, rows_wide written
once.  Networks are untrained ones of the shapes the reference's policy configs give: times do not depend on the values."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cell-num", type=int, default=4)
    ap.add_argument("--cell-size", type=float, default=1.0)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    import bench
    from ebcsim import _abi, actions as ebc_actions
    from ebcsim.batched import BatchedEnv
    from ebcsim.occupancy import OccupancySpec, occupancy_rows_device
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    from ebcsim.train import SarlModule
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
    spec = OccupancySpec(args.cell_num, args.cell_size, args.channels)
    say("# tools/om_bench.py --envs %d --blocks %d --reps %d, %d x %d cells of %g m x %d channels: device ms per call, median "
        "(min .. max) of the blocks; %s" % (E, args.blocks, args.reps, spec.cell_num, spec.cell_num, spec.cell_size, spec.channels,
                                            torch.cuda.get_device_name(0)))

    def net_of(width):
        torch.manual_seed(11)
        m = SarlModule(width, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 6)
        return SarlValueNet({k: v.detach() for k, v in m.state_dict().items()}, device="cuda:0")
    params, batch = bench.build_batch("metric", E, 0)
    params.with_agent_type = 1
    env = BatchedEnv(params, E, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    space = ebc_actions.build_action_space(float(batch.robot[0, 7]))
    A, R, T, W = len(space), env.R, env.T, spec.width
    for om in (None, spec):
        net = net_of(T + (W if om else 0))
        pol = DeviceSarlPolicy(net, space, 0.9, om=om)
        med, lo, hi = timed(lambda: pol.decide(env))
        say("decision  %-28s E %d x A %d x R %d x %3d columns: %8.3f ms (%.3f .. %.3f)" % (
            "with maps (OM-SARL)" if om else "without maps (SARL)", E, A, R, T + (W if om else 0), med, lo, hi))
        if om is None:
            med, lo, hi = timed(lambda: env.lookahead_device(pol._acts, pol._bufs, human_policy=_abi.HUMAN_ORCA))
            say("  of which the look-ahead sweep alone:                                       %8.3f ms (%.3f .. %.3f)" % (med, lo, hi))
            continue
        st = net.refine_stats or {}
        say("  mlp1 of width %d ran in the library (general block: the streamed mlp1 takes one input tile): %d matrix-core forwards, "
            "%d float32 forwards; bound violations %d" % (T + W, getattr(net, "native_forwards", 0),
                                                          getattr(net, "native_exact_forwards", 0), st.get("bound_violations", 0)))
        rows, ob = pol._bufs["rows_rotated"], pol._bufs["next_ob"]
        med, lo, hi = timed(lambda: occupancy_rows_device(ob, None, spec, rows=rows, wide_out=pol._wide, want_om=False))
        moved = rows.numel() * 4 + pol._wide.numel() * 4
        say("  ebc_occupancy_rows alone (maps + %d wide rows of %d floats):          %8.3f ms (%.3f .. %.3f)  %.2f TB/s of %.0f MB "
            "(the look-ahead's row output: 4.1 TB/s, DESIGN §3)" % (E * A * R, T + W, med, lo, hi, moved / med / 1e9, moved / 1e6))
        med, lo, hi = timed(lambda: occupancy_rows_device(ob, None, spec))
        say("  ebc_occupancy_rows, the maps alone (om [E][R][%d]):                          %8.3f ms (%.3f .. %.3f)" % (W, med, lo, hi))
    env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
