#!/usr/bin/env python3
"""Device time of one SAIL gradient at `--envs` envs x `--adults` adults on device-generated scenes, two ways on the same
inputs and the same device — the kernel (ebc_sail_grad: forward, backward and the reduction of the chunk partials) and
torch autograd of SailModule (forward, loss, backward) — and of a full optimizer step each way (loss_and_grad, Adam, the
weights handed back to the network).

    python3 tools/sail_train_bench.py [--envs 4096] [--adults 5] [--blocks 7] [--reps 5] [--out profiles/sail_train.txt]

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
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--adults", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _capi, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import SailModule
    from ebcsim.sail_train import SailTrainer
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
    say("# tools/sail_train_bench.py --envs %d --adults %d --blocks %d --reps %d: device ms per call, median (min .. max) of "
        "the blocks; %s; library %s" % (E, N, args.blocks, args.reps, torch.cuda.get_device_name(0), os.path.basename(_capi.LIB_PATH)))
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
    dev = torch.device("cuda:0")
    robot = torch.empty((E, 9), dtype=torch.float64, device=dev)
    ob = torch.empty((E, env.R, 5), dtype=torch.float64, device=dev)
    n_rows = torch.empty((E,), dtype=torch.int64, device=dev)
    target = torch.empty((E, 2), dtype=torch.float64, device=dev)
    env.robot_state_device(robot)
    env.observe_ob_device(ob)
    env.row_counts_device(n_rows)
    env.robot_orca_device(target, 0.15)  # the demonstrator's action on the same states
    torch.cuda.synchronize()
    assert int((n_rows != N).sum()) == 0, "the generated scenes do not have %d rows each" % N
    torch.manual_seed(11)
    sd = SailModule(N).state_dict()
    native, auto = SailTrainer(sd, device=dev, native=True), SailTrainer(sd, device=dev, native=False)
    scale = 1.0 / E

    def grad(tr):
        return tr.loss_and_grad(robot, ob, target, n_rows, grad_scale=scale)

    def step(tr):
        grad(tr)
        tr.step()

    ln, cn = grad(native)
    la, ca = grad(auto)
    torch.cuda.synchronize()
    gn, ga = native.flat.grad, auto.flat.grad
    say("one batch both ways: count %d / %d, loss_sum %.9g / %.9g, largest |kernel - autograd| of the gradient %.3g (largest entry %.3g)"
        % (int(cn), int(ca), float(ln), float(la), float((gn - ga).abs().max()), float(ga.abs().max())))
    k_med, lo, hi = timed(lambda: grad(native))
    say("ebc_sail_grad (forward + backward + reduction)           E %d x N %d: %8.3f ms (%.3f .. %.3f)" % (E, N, k_med, lo, hi))
    a_med, lo, hi = timed(lambda: grad(auto))
    say("torch autograd of SailModule (forward, loss, backward, repack)      : %8.3f ms (%.3f .. %.3f)" % (a_med, lo, hi))
    say("autograd / kernel: %.2f x" % (a_med / k_med))
    ks_med, lo, hi = timed(lambda: step(native))
    say("full step, kernel   (loss_and_grad, Adam on the flat image, set_packed): %8.3f ms (%.3f .. %.3f)" % (ks_med, lo, hi))
    as_med, lo, hi = timed(lambda: step(auto))
    say("full step, autograd (loss_and_grad, Adam on the flat image, set_packed): %8.3f ms (%.3f .. %.3f)" % (as_med, lo, hi))
    say("full step autograd / kernel: %.2f x" % (as_med / ks_med))
    env.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
