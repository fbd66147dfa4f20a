#!/usr/bin/env python3
"""What the world-frame records of a K-step window cost (ebc_step_k_world), and that plain ebc_step_k costs what it did:

    python3 tools/step_k_world_bench.py [--envs 4096] [--K 50] [--repeats 7] [--measure a b c] [--parent-lib OLD_LIBEBCSIM_SO]
                                        [--demo-steps 120] [--demo-steps-per-call 40] [--out profiles/step_k_world.txt]

(a) plain ebc_step_k (ORCA robot; state_rotated + reward / done / info), per-step and one-launch, of the library built
    from the parent commit (--parent-lib, loaded through EBCSIM_LIB) against this tree's: five pairs of child processes,
    parent and tree alternating, each the median of `--repeats` calls.  "No slowdown" = this tree's medians inside the
    parent's own min .. max over its five processes; a median outside it is printed as SLOWER (or faster).  Skipped
    without --parent-lib.
(b) ebc_step_k_world (the same outputs plus world_robot and world_ob) against ebc_step_k, both forms, alternating call
    by call in one process.
(c) sail_train.collect_sail_demos at 4096 envs x 5 adults: the Python loop, windows per step, windows in one launch;
    device events around the whole collection, alternating; and the three dictionaries compared.

The metric config (10 humans, 4 walls) on device-generated scenes with auto-reset from a generated pool for (a) and (b);
times are HIP events around the whole call, us per step; two warm-up calls first."""
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

PLAIN = ("state_rotated", "reward", "done", "info")


def timed(torch, fn, per):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / per * 1e3  # us


def alternating(torch, forms, repeats, per, before=None):
    """forms: {name: callable}; two warm-up rounds, then `repeats` rounds, the forms one after the other in every round
    -> {name: [us]}"""
    times = {k: [] for k in forms}
    for it in range(2 + repeats):
        for name, fn in forms.items():
            if before:
                before()
            t = timed(torch, fn, per)
            if it >= 2:
                times[name].append(t)
    return times


def fmt(ts):
    return "%9.2f us (%.2f .. %.2f)" % (statistics.median(ts), min(ts), max(ts))


def metric_env(E, adults=None):
    from ebcsim import config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    params = ebc_config.params_from_config(cfg, pol, **({"policy": "sail"} if adults else {}))
    sc = ebc_scene.SceneConfig.from_config(cfg)
    if adults:
        sc.adult_num, sc.bicycle_num, sc.children_num, sc.num_circles, sc.num_walls = adults, 0, 0, 0, 0
    gen = ebc_scene.gen_struct(sc, "test")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    return env, gen


def plain_child(args):
    """One process of measure (a): plain ebc_step_k of whatever library EBCSIM_LIB names -> one JSON line"""
    import torch
    from ebcsim import _abi
    E, K = args.envs, args.K
    env, gen = metric_env(E)
    outs = env.alloc_step_k_outputs(K, PLAIN)
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)

    def again():
        env.generate_reset(gen, 1000)
        env.generate_pool(gen, 100000, E)
    forms = {"per_step": lambda: env.step_k_device(outs, K, flags=_abi.FLAG_AUTO_RESET, **kw),
             "one_launch": lambda: env.step_k_device(outs, K, flags=_abi.FLAG_AUTO_RESET | _abi.FLAG_ONE_LAUNCH, **kw)}
    t = alternating(torch, forms, args.repeats, K, again)
    env.close()
    print(json.dumps({k: statistics.median(v) for k, v in t.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser(description="ebc_step_k_world against ebc_step_k, and collect_sail_demos in windows")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--measure", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--parent-lib", default=None, help="libebcsim.so built from the parent commit, for (a)")
    ap.add_argument("--demo-steps", type=int, default=120, help="(c): the demonstration length, tools/train_sail.py's default")
    ap.add_argument("--demo-steps-per-call", type=int, default=40)
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.repeats < 1:
        ap.error("--repeats must be at least 1")
    if args.plain_child:
        return plain_child(args)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    E, K = args.envs, args.K
    if "a" in args.measure and args.parent_lib:
        # before this process opens the device: one child at a time, each with a library of its own
        res = {"parent": [], "tree": []}
        for pair in range(5):
            for who in ("parent", "tree"):
                envv = dict(os.environ)
                envv.pop("EBCSIM_LIB", None)
                if who == "parent":
                    envv["EBCSIM_LIB"] = os.path.abspath(args.parent_lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--envs", str(E), "--K", str(K),
                                    "--repeats", str(args.repeats)], env=envv, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("measure (a), %s library: exit %d\n%s" % (who, r.returncode, r.stderr[-2000:]))
                res[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
        say("# (a) plain ebc_step_k, %d envs x 10 humans, K %d, ORCA robot, state_rotated + reward / done / info: five pairs of "
            "processes, parent and tree alternating, each the median of %d calls; us per step" % (E, K, args.repeats))
        for form in ("per_step", "one_launch"):
            p, t = [r[form] for r in res["parent"]], [r[form] for r in res["tree"]]
            say("(a) %-10s parent medians %s" % (form, " ".join("%.2f" % x for x in p)))
            say("(a) %-10s tree   medians %s" % (form, " ".join("%.2f" % x for x in t)))
            lo, hi = min(p), max(p)
            inside = [lo <= x <= hi for x in t]
            verdict = "no slowdown: every tree median inside the parent's spread" if all(inside) else (
                "SLOWER: %d of 5 tree medians above the parent's spread" % sum(x > hi for x in t) if any(x > hi for x in t)
                else "%d of 5 tree medians below the parent's spread (faster), none above" % sum(x < lo for x in t))
            say("(a) %-10s parent spread %.2f .. %.2f; tree %.2f .. %.2f, median of medians %.2f vs %.2f: %s" % (
                form, lo, hi, min(t), max(t), statistics.median(t), statistics.median(p), verdict))
    elif "a" in args.measure:
        say("# (a) skipped: no --parent-lib")

    import torch
    from ebcsim import _abi
    say("# tools/step_k_world_bench.py --envs %d --K %d --repeats %d; %s" % (E, K, args.repeats, torch.cuda.get_device_name(0)))
    if "b" in args.measure:
        env, gen = metric_env(E)
        plain = env.alloc_step_k_outputs(K, PLAIN)
        world = dict(plain, **env.alloc_step_k_outputs(K, ("world_robot", "world_ob")))
        kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)

        def again():
            env.generate_reset(gen, 1000)
            env.generate_pool(gen, 100000, E)
        say("# (b) %d envs x 10 humans (R = %d rows), K %d, ORCA robot: ebc_step_k_world (+ world_robot, world_ob: %.1f MB per call) "
            "against ebc_step_k with the same other outputs, alternating; us per step, median (min .. max)" % (
                E, env.R, K, K * E * (9 + env.R * 5) * 8 / 1e6))
        for form, extra in (("per-step", 0), ("one-launch", _abi.FLAG_ONE_LAUNCH)):
            fl = _abi.FLAG_AUTO_RESET | extra
            t = alternating(torch, {"plain": lambda: env.step_k_device(plain, K, flags=fl, **kw),
                                    "world": lambda: env.step_k_device(world, K, flags=fl, **kw)}, args.repeats, K, again)
            ratio = statistics.median(t["world"]) / statistics.median(t["plain"])
            say("(b) %-10s ebc_step_k %s   ebc_step_k_world %s   world / plain %.3f x%s" % (
                form, fmt(t["plain"]), fmt(t["world"]), ratio, "  SLOWER" if ratio > 1.0 else ""))
        env.close()
    if "c" in args.measure:
        from ebcsim.sail_train import collect_sail_demos
        env, gen = metric_env(E, adults=5)
        steps, Kc = args.demo_steps, args.demo_steps_per_call
        got = {}

        def again():
            env.generate_reset(gen, 1000)
            env.generate_pool(gen, 100000, 4 * E)

        def form(name, **kw):
            def run():
                got[name] = collect_sail_demos(env, steps, **kw)
            return run
        forms = {"loop": form("loop"), "windows": form("windows", steps_per_call=Kc),
                 "one-launch": form("one-launch", steps_per_call=Kc, one_launch=True)}
        t = alternating(torch, forms, args.repeats, steps, again)
        say("# (c) collect_sail_demos, %d envs x 5 adults, %d steps, windows of %d: device events around the whole collection "
            "(the ReachGoal filter included), alternating; us per step, median (min .. max)" % (E, steps, Kc))
        base = statistics.median(t["loop"])
        for name in forms:
            r = statistics.median(t[name]) / base
            say("(c) %-10s %s   / loop %.3f x%s" % (name, fmt(t[name]), r, "  SLOWER" if r > 1.0 else ""))
        same = all(got[n]["steps"] == got["loop"]["steps"] and got[n]["episodes"] == got["loop"]["episodes"] and all(
            torch.equal(got[n][k].view(torch.int64), got["loop"][k].view(torch.int64)) for k in ("robot", "ob", "n_rows", "target"))
            for n in ("windows", "one-launch"))
        say("(c) the three dictionaries: %s; %d steps kept of %d episodes" % (
            "the same bytes" if same else "DIFFERENT", got["loop"]["steps"], got["loop"]["episodes"]))
        env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
