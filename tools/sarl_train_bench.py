#!/usr/bin/env python3
"""Time of one SARL gradient, two ways on the same inputs and the same device: the kernel (ebc_sarl_grad: forward of every
row, softmax, backward and the reduction of the chunk partials) and torch autograd of SarlModule (forward, MSE loss,
backward), at the reference's batch of 100 states and at 4096, with 5 and 10 rows per state, T = 13; and a full optimizer
step through SarlTrainer against ebcsim.train.DataParallelTrainer.optimize_batch(1), what run_training takes per step.

    python3 tools/sarl_train_bench.py [--blocks 7] [--reps 20] [--out profiles/sarl_train.txt] [--passes]

--passes instead times the pass form of the kernel (states_per_pass): 4, 2 and 1 states of a chunk at a time against the
whole chunk at the shapes above, and states_per_pass="auto" at 16, 24 and 30 rows per state against torch autograd.

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

SHAPES = [(100, 5), (100, 10), (4096, 5), (4096, 10)]
WIDE_SHAPES = [(100, 16), (100, 24), (100, 30), (4096, 16), (4096, 24), (4096, 30)]  # --passes: past the whole chunk's limit
DIMS = dict(input_dim=13, mlp1_dims=[150, 100], mlp2_dims=[100, 50], mlp3_dims=[150, 100, 100, 1], attention_dims=[100, 100, 1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--passes", action="store_true", help="time the pass form (states_per_pass) instead")
    args = ap.parse_args()
    import torch
    from ebcsim import _capi
    from ebcsim.sarl_train import SarlTrainer
    from ebcsim.train import DataParallelTrainer, SarlModule
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
    say("# tools/sarl_train_bench.py --blocks %d --reps %d: ms per call, median (min .. max) of the blocks by stream events, "
        "and the host clock's median; network 13 | 150-100 | 100-50 | 100-100-1 | 150-100-100-1, global state; %s; library %s"
        % (args.blocks, args.reps, torch.cuda.get_device_name(0), os.path.basename(_capi.LIB_PATH)))
    torch.manual_seed(11)
    sd = SarlModule(**DIMS).state_dict()
    native = SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=True)
    auto = SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=False)
    module = SarlModule(**DIMS).to(dev)
    module.load_state_dict(sd)
    dp_model = SarlModule(**DIMS).to(dev)
    dp_model.load_state_dict(sd)
    say("# ebc_sarl_net_grad_max_rows = %d" % native.net.grad_max_rows())
    if args.passes:
        say("# ebc_sarl_net_grad_max_rows_at(4, 2, 1) = %s" % ", ".join(str(native.net.grad_max_rows(S)) for S in (4, 2, 1)))
        by_pass = {S: SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=True, states_per_pass=S) for S in (4, 2, 1, "auto")}
    for B, R in SHAPES + WIDE_SHAPES if args.passes else []:
        g = torch.Generator(device=dev).manual_seed(1000 * B + R)
        rows = torch.randn((B, R, 13), generator=g, device=dev)
        target = 0.5 * torch.randn((B,), generator=g, device=dev)
        if (B, R) in SHAPES:
            native.loss_and_grad(rows, target, grad_scale=2.0 / B)
            whole = native.flat.grad.clone()
            k0 = timed(lambda: native.loss_and_grad(rows, target, grad_scale=2.0 / B))
            say("B %4d R %2d  ebc_sarl_grad, the whole chunk (states_per_pass unset) : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + k0))
            for S in (4, 2, 1):
                tr = by_pass[S]
                tr.loss_and_grad(rows, target, grad_scale=2.0 / B)
                same = bool(torch.equal(tr.flat.grad.view(torch.int32), whole.view(torch.int32)))
                k = timed(lambda: tr.loss_and_grad(rows, target, grad_scale=2.0 / B))
                say("B %4d R %2d  ebc_sarl_grad, states_per_pass = %d                       : %8.3f ms (%.3f .. %.3f), host clock %.3f ms; "
                    "%.2f x the whole chunk; the same bytes: %s" % ((B, R, S) + k + (k[0] / k0[0], same)))
            continue
        tr = by_pass["auto"]

        def bare():
            for p in module.parameters():
                p.grad = None
            torch.nn.functional.mse_loss(module(rows), target).backward()
        k = timed(lambda: tr.loss_and_grad(rows, target, grad_scale=2.0 / B))
        a = timed(bare)
        say("B %4d R %2d  ebc_sarl_grad, states_per_pass = auto (%d)                : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R, tr.passes.of(R)) + k))
        say("B %4d R %2d  torch autograd of SarlModule (forward, MSE, backward)    : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + a))
        say("B %4d R %2d  autograd / kernel: %.2f x by events, %.2f x by the host clock" % (B, R, a[0] / k[0], a[3] / k[3]))
    for B, R in [] if args.passes else SHAPES:
        g = torch.Generator(device=dev).manual_seed(1000 * B + R)
        rows = torch.randn((B, R, 13), generator=g, device=dev)
        target = 0.5 * torch.randn((B,), generator=g, device=dev)
        scale = 2.0 / B

        class Fixed(object):  # the batch as DataParallelTrainer's memory
            def sample(self, bs, generator=None):
                return rows, target
        dp = DataParallelTrainer(dp_model, Fixed(), B, "sgd", 1e-3)

        def bare():
            """what the reference's optimize_batch does between zero_grad and step"""
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
        say("B %4d R %2d: count %d / %d, loss_sum %.9g / %.9g, largest |kernel - autograd| of the gradient %.3g (largest entry %.3g)"
            % (B, R, int(cn), int(ca), float(ln), float(la), float((gn - ga).abs().max()), float(ga.abs().max())))
        k = timed(lambda: grad(native))
        say("B %4d R %2d  ebc_sarl_grad (forward, softmax, backward, reduction)        : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + k))
        a = timed(bare)
        say("B %4d R %2d  torch autograd of SarlModule (forward, MSE, backward)         : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + a))
        say("B %4d R %2d  autograd / kernel: %.2f x by events, %.2f x by the host clock" % (B, R, a[0] / k[0], a[3] / k[3]))
        ks = timed(lambda: step(native))
        say("B %4d R %2d  full step, SarlTrainer native (loss_and_grad, SGD on the flat image, set_packed) : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + ks))
        as_ = timed(lambda: step(auto))
        say("B %4d R %2d  full step, SarlTrainer autograd (unpack, autograd, repack, SGD)                  : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + as_))
        ds = timed(lambda: dp.optimize_batch(1))
        say("B %4d R %2d  full step, DataParallelTrainer.optimize_batch(1)                                 : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((B, R) + ds))
        say("B %4d R %2d  DataParallelTrainer / SarlTrainer native: %.2f x by events, %.2f x by the host clock" % (B, R, ds[0] / ks[0], ds[3] / ks[3]))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
