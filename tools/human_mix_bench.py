#!/usr/bin/env python3
"""What humans on a policy per entity type cost (EBC_HUMAN_BY_TYPE, include/ebcsim.h at ebc_set_human_policies).

    python tools/human_mix_bench.py [--parent-lib PATH] [--envs 4096,16384] [--reps 7] [--steps 2000] [--window 50]

The bench's metric scenes (bench.build_batch: 10 humans of types 4 / 3 / 3 and 8 static rows per env, auto-reset, robot on
its linear policy, the outputs bench.py asks for).  One child process per library and batch size, the children of the two
libraries alternating; inside a child every form has a handle of its own reset from the same scenes, and the forms
ALTERNATE in blocks of --steps steps timed with device events after a warm-up:

    orca       human_policy = EBC_HUMAN_ORCA (the headline step; the only form the parent's library has)
    all_orca   EBC_HUMAN_BY_TYPE, a table of three EBC_HUMAN_ORCA: the mixed kernel with nothing to skip
    bikes      EBC_HUMAN_BY_TYPE, bicycles on linear (3 of 10 humans solve no LP)
    linear     EBC_HUMAN_BY_TYPE, everybody on linear

then a window of --window steps (ebc_step_k, robot on its linear policy) in the per-step and the one-launch form for
`orca` and `bikes`.  Printed per form: the median and the min .. max of the blocks, in microseconds per step."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eb-cadrl_amd"))
sys.path.insert(0, ROOT)

FORMS = {"orca": None, "all_orca": "ooo", "bikes": "olo", "linear": "lll"}


def child(args):
    import torch
    import bench
    from ebcsim import _abi, _capi
    from ebcsim.batched import BatchedEnv
    mixed_ok = hasattr(_capi.lib(), "ebc_set_human_policies")
    forms = [f for f in FORMS if f == "orca" or mixed_ok]
    E = args.child
    params, batch = bench.build_batch("metric", E, 0)
    code = {"o": _abi.HUMAN_ORCA, "l": _abi.HUMAN_LINEAR}
    envs, outs, kws = {}, {}, {}
    for f in forms:
        env = BatchedEnv(params, E, batch.N, batch.S)
        env.reset(batch)
        env.use_torch_stream()
        if FORMS[f]:
            env.set_human_policies(*[code[c] for c in FORMS[f]])
        envs[f] = env
        outs[f] = env.alloc_step_outputs(("reward", "done", "info", "obs_rotated"))
        kws[f] = dict(human_policy=_abi.HUMAN_BY_TYPE if FORMS[f] else _abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR,
                      flags=_abi.FLAG_AUTO_RESET)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, n):
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n  # us per call

    res = {"lib": os.environ.get("EBCSIM_LIB") or "tree", "envs": E, "step_us": {f: [] for f in forms}, "window_us_per_step": {}}
    for f in forms:
        timed(lambda: envs[f].step_device(outs[f], **kws[f]), args.warmup)
    for _ in range(args.reps):
        for f in forms:
            res["step_us"][f].append(timed(lambda: envs[f].step_device(outs[f], **kws[f]), args.steps))
    K = args.window
    wforms = [(f, one) for f in ("orca", "bikes") if f in forms for one in (0, 1)]
    wouts = {f: envs[f].alloc_step_k_outputs(K, ("reward", "done", "info", "obs_rotated")) for f, _ in wforms}
    for f, one in wforms:
        res["window_us_per_step"]["%s %s" % (f, "one-launch" if one else "per-step")] = []
    for r in range(args.reps + 1):
        for f, one in wforms:
            kw = dict(kws[f], flags=_abi.FLAG_AUTO_RESET | (_abi.FLAG_ONE_LAUNCH if one else 0))
            t = timed(lambda: envs[f].step_k_device(wouts[f], K, **kw), 10) / K
            if r:  # the first round warms the window's kernels
                res["window_us_per_step"]["%s %s" % (f, "one-launch" if one else "per-step")].append(t)
    for env in envs.values():
        env.synchronize()
    print("RESULT " + json.dumps(res), flush=True)


def summary(v):
    s = sorted(v)
    return "%8.2f  (%.2f .. %.2f, %d blocks)" % (s[len(s) // 2], s[0], s[-1], len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libebcsim.so of the parent commit, built into a side directory")
    ap.add_argument("--envs", default="4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="children per library and batch size, alternating")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = [("tree", None)] + ([("parent", args.parent_lib)] if args.parent_lib else [])
    for E in [int(x) for x in args.envs.split(",")]:
        got = {}
        for _ in range(args.rounds):
            for name, path in libs:
                env = dict(os.environ)
                env.pop("EBCSIM_LIB", None)
                if path:
                    env["EBCSIM_LIB"] = os.path.abspath(path)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", str(E), "--reps", str(args.reps), "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--window", str(args.window)]
                out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=600, check=True).stdout
                r = json.loads([line for line in out.splitlines() if line.startswith("RESULT ")][-1][7:])
                for kind in ("step_us", "window_us_per_step"):
                    for f, v in r[kind].items():
                        got.setdefault((kind, name, f), []).extend(v)
        print("== %d envs x 10 humans (4 / 3 / 3) + 8 static rows, us per step: median (min .. max)" % E)
        for (kind, name, f), v in got.items():
            print("%-20s %-7s %-22s %s" % ("ebc_step" if kind == "step_us" else "ebc_step_k K=%d" % args.window, name, f, summary(v)), flush=True)


if __name__ == "__main__":
    main()
