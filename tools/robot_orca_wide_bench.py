#!/usr/bin/env python3
"""What the robot's own ORCA solve costs by observation width, and that the at-most-32-row kernel costs what it did:

    python3 tools/robot_orca_wide_bench.py [--envs 4096] [--repeats 9] [--calls 20] [--K 20] [--measure a b c]
                                           [--parent-lib OLD_LIBEBCSIM_SO] [--out profiles/robot_orca_wide.txt]

(a) ebc_robot_orca at R = N + S = 10 and 32 rows (orca_robot_kernel, a lane per row) and at 33, 44, 64 and 128 rows
    (orca_robot_wide_kernel: selection of the 10 nearest rows, then the same solve), one process, the shapes one after
    the other in every round.
(b) an imitation window: ebc_step_k, K steps, EBC_ROBOT_ORCA with the persistent simulator, auto-reset, at (N, S) = (14, 30).
(c) R = 10 and R = 32 with the library built from the parent commit (--parent-lib, loaded through EBCSIM_LIB) against
    this tree's: five pairs of child processes, parent and tree alternating, the first of a pair swapped from pair to
    pair.  "No slowdown" = this tree's median inside
    the parent's own min .. max over its five processes; a median outside it is printed as SLOWER (or faster).  Skipped
    without --parent-lib.

Scenes: humans and static rows uniform in a 10 m box around the robot's path, radius 0.3, every row in range of the
robot (neighbor_dist 10), so the selection always has more than 10 candidates past R = 10.  Times are HIP events around
`--calls` back-to-back calls (a single call is a few microseconds), us per call, the median of `--repeats` such regions
after two warm-up rounds; (b) times one call of K steps, us per step."""
import argparse
import configparser
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)

SHAPES = {10: (10, 0), 32: (14, 18), 33: (14, 19), 44: (14, 30), 64: (14, 50), 128: (33, 95)}  # R -> (humans, static rows)
NARROW = (10, 32)


def params_of():
    from ebcsim import config as ebc_config
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_plain.config"))
    return ebc_config.params_from_config(cfg, pol)


def crowd(seed, E, N, S):
    import numpy as np
    from ebcsim.scene import SceneBatch
    rs = np.random.RandomState(seed)
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = SceneBatch(E, N, S, np.full(E, N, np.int32), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                   np.zeros((E, N), np.uint8), np.full(E, S, np.int32), f(E, max(S, 1)), f(E, max(S, 1)), f(E, max(S, 1)), None,
                   f(E, 9))
    for k in ("px", "py", "gx", "gy"):
        getattr(b, k)[:] = rs.uniform(-5, 5, (E, N))
    b.vx[:], b.vy[:] = rs.uniform(-0.5, 0.5, (E, N)), rs.uniform(-0.5, 0.5, (E, N))
    b.radius[:], b.v_pref[:] = 0.3, 1.0
    if S:
        b.spx[:], b.spy[:], b.sradius[:] = rs.uniform(-5, 5, (E, S)), rs.uniform(-5, 5, (E, S)), 0.3
    b.robot[:] = [0.0, -4.0, 0.0, 0.0, 0.3, 0.0, 4.0, 1.0, 1.5707963267948966]
    b.robot[:, 0] = rs.uniform(-1, 1, E)
    return b


def timed(torch, fn, per):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / per * 1e3  # us


def fmt(ts):
    return "%8.2f us (%.2f .. %.2f)" % (statistics.median(ts), min(ts), max(ts))


def solve_times(args, widths):
    """{R: [us per ebc_robot_orca call]} at the given widths, the widths one after the other in every round"""
    import torch
    from ebcsim.batched import BatchedEnv
    params = params_of()
    envs = {}
    for R in widths:
        N, S = SHAPES[R]
        env = BatchedEnv(params, args.envs, N, S)
        env.use_torch_stream()
        env.reset(crowd(100 + R, args.envs, N, S))
        envs[R] = (env, torch.zeros((args.envs, 2), dtype=torch.float64, device="cuda:0"))

    def calls(R):
        env, act = envs[R]
        for _ in range(args.calls):
            env.robot_orca_device(act, 0.15)
    times = {R: [] for R in widths}
    for it in range(2 + args.repeats):
        for R in widths:
            t = timed(torch, lambda: calls(R), args.calls)
            if it >= 2:
                times[R].append(t)
    for env, _ in envs.values():
        env.close()
    return times


def narrow_child(args):
    """One process of measure (c): whatever library EBCSIM_LIB names -> one JSON line"""
    t = solve_times(args, NARROW)
    print(json.dumps({str(R): statistics.median(v) for R, v in t.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser(description="the robot's ORCA solve by observation width")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back ebc_robot_orca calls inside one timed region")
    ap.add_argument("--K", type=int, default=20, help="(b): steps of the imitation window")
    ap.add_argument("--measure", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--parent-lib", default=None, help="libebcsim.so built from the parent commit, for (c)")
    ap.add_argument("--narrow-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.repeats < 7:
        ap.error("--repeats must be at least 7")
    if args.narrow_child:
        return narrow_child(args)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    E = args.envs
    if "c" in args.measure and args.parent_lib:
        # before this process opens the device: one child at a time, each with a library of its own
        res = {"parent": [], "tree": []}
        for pair in range(5):
            for who in (("parent", "tree") if pair % 2 == 0 else ("tree", "parent")):  # neither is always the warmer one
                envv = dict(os.environ)
                envv.pop("EBCSIM_LIB", None)
                if who == "parent":
                    envv["EBCSIM_LIB"] = os.path.abspath(args.parent_lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--narrow-child", "--envs", str(E), "--repeats",
                                    str(args.repeats), "--calls", str(args.calls)], env=envv, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise RuntimeError("measure (c), %s library: exit %d\n%s" % (who, r.returncode, r.stderr[-2000:]))
                res[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
        say("# (c) ebc_robot_orca at most 32 rows (orca_robot_kernel), %d envs: five pairs of processes, parent and tree "
            "alternating, each the median of %d regions of %d calls; us per call" % (E, args.repeats, args.calls))
        for R in NARROW:
            p, t = [r[str(R)] for r in res["parent"]], [r[str(R)] for r in res["tree"]]
            say("(c) R %-3d parent medians %s" % (R, " ".join("%.2f" % x for x in p)))
            say("(c) R %-3d tree   medians %s" % (R, " ".join("%.2f" % x for x in t)))
            lo, hi, med = min(p), max(p), statistics.median(t)
            verdict = "inside the parent's spread" if lo <= med <= hi else ("SLOWER than the parent's spread" if med > hi else "faster than the parent's spread")
            say("(c) R %-3d parent %.2f .. %.2f (median %.2f), tree median %.2f: %s" % (R, lo, hi, statistics.median(p), med, verdict))
    if "a" in args.measure:
        widths = sorted(SHAPES)
        t = solve_times(args, widths)
        say("# (a) ebc_robot_orca, %d envs, safety space 0.15: median (min .. max) of %d regions of %d calls; us per call" % (E, args.repeats, args.calls))
        base = statistics.median(t[32]) / 32
        for R in widths:
            med = statistics.median(t[R])
            kernel = "orca_robot_kernel" if R <= 32 else "orca_robot_wide_kernel"
            note = ""
            if R > 32:
                note = ", %.3f us per row against %.3f at R = 32: %s per row" % (med / R, base, "SLOWER" if med / R > base else "faster")
            say("(a) R %-3d (N %2d, S %2d) %-22s %s%s" % (R, SHAPES[R][0], SHAPES[R][1], kernel, fmt(t[R]), note))
    if "b" in args.measure:
        import torch
        from ebcsim import _abi
        from ebcsim.batched import BatchedEnv
        N, S = SHAPES[44]
        env = BatchedEnv(params_of(), E, N, S)
        env.use_torch_stream()
        first, pool = crowd(7, E, N, S), crowd(8, E, N, S)
        outs = env.alloc_step_k_outputs(args.K, ("state_rotated", "reward", "done", "info"))
        ts = []
        for it in range(2 + args.repeats):
            env.reset(first)
            env.set_scene_pool(pool)
            env.robot_orca_sim(True)
            t = timed(torch, lambda: env.step_k_device(outs, args.K, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA,
                                                       flags=_abi.FLAG_AUTO_RESET, robot_safety_space=0.15), args.K)
            if it >= 2:
                ts.append(t)
        env.close()
        say("# (b) imitation window: ebc_step_k per step, EBC_ROBOT_ORCA with the persistent simulator, auto-reset, %d envs, "
            "(N, S) = (%d, %d), K %d; us per step (state + demonstrator + fused ORCA step)" % (E, N, S, args.K))
        say("(b) K %d window %s" % (args.K, fmt(ts)))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
