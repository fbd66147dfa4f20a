#!/usr/bin/env python3
"""Time of one CADRL gradient, two ways on the same inputs and the same device: the kernel (ebc_cadrl_grad: forward of
every row, minimum, backward and the reduction of the chunk partials) and torch autograd of CadrlModule (forward, minimum
over the rows, MSE loss, backward), at the reference's batch of 100 states and at 4096, with 1 and 5 rows per state; and a
full optimizer step each way through CadrlTrainer.

    python3 tools/cadrl_train_bench.py [--blocks 7] [--reps 20] [--out profiles/cadrl_train.txt]

Warm-up first, then the median over `--blocks` blocks of `--reps` back-to-back calls.  Two clocks per block: a pair of
events on the stream (what the device sees from the first kernel's start to the last one's end, host gaps between the
launches included) and the host's clock around the block with a synchronize at its end."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)

SHAPES = [(100, 1), (100, 5), (4096, 1), (4096, 5)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _capi
    from ebcsim.cadrl import CadrlModule
    from ebcsim.cadrl_train import CadrlTrainer
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        dev_ms, host_ms = [], []
        for _ in range(args.blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3 / args.reps)
            dev_ms.append(a.elapsed_time(b) / args.reps)
        return statistics.median(dev_ms), min(dev_ms), max(dev_ms), statistics.median(host_ms)

    dev = torch.device("cuda:0")
    say("# tools/cadrl_train_bench.py --blocks %d --reps %d: ms per call, median (min .. max) of the blocks by stream events, "
        "and the host clock's median; network 13-150-100-100-1; %s; library %s"
        % (args.blocks, args.reps, torch.cuda.get_device_name(0), os.path.basename(_capi.LIB_PATH)))
    torch.manual_seed(11)
    sd = CadrlModule(13, [150, 100, 100, 1]).state_dict()
    native = CadrlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=True)
    auto = CadrlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=False)
    module = CadrlModule.from_state_dict(sd).to(dev)
    for B, R in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1000 * B + R)
        rows = torch.randn((B, R, 13), generator=g, device=dev)
        target = 0.5 * torch.randn((B,), generator=g, device=dev)
        scale = 2.0 / B

        def bare():
            """what the reference's optimize_batch does between zero_grad and step, with the minimum over the rows"""
            for p in module.parameters():
                p.grad = None
            torch.nn.functional.mse_loss(module(rows), target).backward()

        def grad(tr):
            return tr.loss_and_grad(rows, target, grad_scale=scale)

        def step(tr):
            grad(tr)
            tr.step()

        ln, cn = grad(native)
        la, ca = grad(auto)
        torch.cuda.synchronize()
        gn, ga = native.flat.grad, auto.flat.grad
        say("B %4d R %d: count %d / %d, loss_sum %.9g / %.9g, largest |kernel - autograd| of the gradient %.3g (largest entry %.3g)"
            % (B, R, int(cn), int(ca), float(ln), float(la), float((gn - ga).abs().max()), float(ga.abs().max())))
        k = timed(lambda: grad(native))
        say("B %4d R %d  ebc_cadrl_grad (forward, minimum, backward, reduction)   : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + k))
        a = timed(bare)
        say("B %4d R %d  torch autograd of CadrlModule (forward, MSE, backward)   : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + a))
        say("B %4d R %d  autograd / kernel: %.2f x by events, %.2f x by the host clock" % (B, R, a[0] / k[0], a[3] / k[3]))
        ks = timed(lambda: step(native))
        say("B %4d R %d  full step, kernel   (loss_and_grad, SGD on the flat image, set_packed)   : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + ks))
        as_ = timed(lambda: step(auto))
        say("B %4d R %d  full step, autograd (unpack, autograd, repack, SGD on the flat image)    : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + as_))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
