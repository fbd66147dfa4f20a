#!/usr/bin/env python3
"""Time of one SARL gradient in its three forms on the same inputs and the same device: the layer form of the kernel
(ebc_sarl_net_create_layers: layer by layer on the float32 matrix instruction), the chunk form (ebc_sarl_net_create, with
states_per_pass="auto" where the rows need passes; it refuses the x2 and x4 widths) and torch autograd of SarlModule
(forward, MSE loss, backward); and the full optimizer step through SarlTrainer for each.  Networks: the reference widths
(T = 13), x2 (T = 17, eb-cadrl_amd/configs/policy_x2.config) and x4 (T = 13); B in 100, 4096; R in 5, 10, 30.

    python3 tools/sarl_grad_forms_bench.py [--blocks 5] [--reps 20] [--reps-large 3] [--nets ref,x2,x4] [--out profiles/sarl_grad_layers.txt]

Warm-up first, then the median over `--blocks` blocks of back-to-back calls (`--reps` at B = 100, `--reps-large` at 4096)
between a pair of events on the stream; the host clock around the block beside it.  Where a kernel form is slower than
autograd the line says SLOWER."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)

NETS = {"ref": dict(input_dim=13, mlp1_dims=[150, 100], mlp2_dims=[100, 50], mlp3_dims=[150, 100, 100, 1], attention_dims=[100, 100, 1]),
        "x2": dict(input_dim=17, mlp1_dims=[300, 200], mlp2_dims=[200, 100], mlp3_dims=[300, 200, 200, 1], attention_dims=[200, 200, 1]),
        "x4": dict(input_dim=13, mlp1_dims=[600, 400], mlp2_dims=[400, 200], mlp3_dims=[600, 400, 400, 1], attention_dims=[400, 400, 1])}
SHAPES = [(B, R) for B in (100, 4096) for R in (5, 10, 30)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-large", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nets", default="ref,x2,x4")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _abi, _capi
    from ebcsim.sarl_train import SarlFormTrainer, SarlTrainer
    from ebcsim.train import SarlModule
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        dev_ms, host_ms = [], []
        for _ in range(args.blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3 / reps)
            dev_ms.append(a.elapsed_time(b) / reps)
        return statistics.median(dev_ms), min(dev_ms), max(dev_ms), statistics.median(host_ms)

    def versus(t, ref):
        return "%.2f x autograd%s" % (ref[0] / t[0], "" if t[0] <= ref[0] else ", SLOWER")

    dev = torch.device("cuda:0")
    say("# tools/sarl_grad_forms_bench.py --blocks %d --reps %d --reps-large %d: ms per call, median (min .. max) of the blocks by stream "
        "events, and the host clock's median; %s; library %s" % (args.blocks, args.reps, args.reps_large, torch.cuda.get_device_name(0),
                                                                  os.path.basename(_capi.LIB_PATH)))
    for name in args.nets.split(","):
        dims = NETS[name]
        torch.manual_seed(11)
        sd = SarlModule(**dims).state_dict()
        say("# network %s: %d | %s | %s | %s | %s, global state" % (name, dims["input_dim"], dims["mlp1_dims"], dims["mlp2_dims"],
                                                                  dims["attention_dims"], dims["mlp3_dims"]))
        layers = SarlFormTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, grad_form="layers")
        autograd = SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=False)
        try:
            chunk = SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, states_per_pass="auto")
        except _capi.EbcError as e:
            assert e.code == _abi.ERR_UNSUPPORTED
            chunk = None
            say("# network %s: the chunk form refuses it (%s)" % (name, str(e).split(": ", 1)[-1]))
        module = SarlModule(**dims).to(dev)
        module.load_state_dict(sd)
        for B, R in SHAPES:
            reps = args.reps if B <= 100 else args.reps_large
            g = torch.Generator(device=dev).manual_seed(1000 * B + R)
            rows = torch.randn((B, R, dims["input_dim"]), generator=g, device=dev)
            target = 0.5 * torch.randn((B,), generator=g, device=dev)
            scale, tag = 2.0 / B, "%-3s B %4d R %2d " % (name, B, R)

            def bare():
                for p in module.parameters():
                    p.grad = None
                torch.nn.functional.mse_loss(module(rows), target).backward()

            def grad(tr):
                return tr.loss_and_grad(rows, target, grad_scale=scale)

            def step(tr):
                grad(tr)
                tr.step()
            a = timed(bare, reps)
            say(tag + " torch autograd of SarlModule (forward, MSE, backward)  : %9.3f ms (%.3f .. %.3f), host clock %.3f ms" % a)
            grad(layers)
            k = timed(lambda: grad(layers), reps)
            say(tag + " ebc_sarl_grad, layer form                              : %9.3f ms (%.3f .. %.3f), host clock %.3f ms; " % k + versus(k, a))
            c = None
            if chunk is not None and R <= chunk.grad_max_rows():
                grad(chunk)
                same = bool(torch.equal(chunk.flat.grad.view(torch.int32), layers.flat.grad.view(torch.int32)))
                c = timed(lambda: grad(chunk), reps)
                say(tag + " ebc_sarl_grad, chunk form (states_per_pass %d)          : %9.3f ms (%.3f .. %.3f), host clock %.3f ms; "
                    % ((chunk.passes.of(R),) + c) + versus(c, a) + "; layer form %.2f x the chunk form%s; the same bytes: %s"
                    % (c[0] / k[0], "" if k[0] <= c[0] else ", SLOWER", same))
            elif chunk is not None:
                say(tag + " ebc_sarl_grad, chunk form: R is past its %d rows" % chunk.grad_max_rows())
            sa = timed(lambda: step(autograd), reps)
            say(tag + " full step, SarlTrainer autograd                        : %9.3f ms (%.3f .. %.3f), host clock %.3f ms" % sa)
            sk = timed(lambda: step(layers), reps)
            say(tag + " full step, SarlFormTrainer, layer form                 : %9.3f ms (%.3f .. %.3f), host clock %.3f ms; " % sk + versus(sk, sa))
            if c is not None:
                sc = timed(lambda: step(chunk), reps)
                say(tag + " full step, SarlTrainer chunk form                      : %9.3f ms (%.3f .. %.3f), host clock %.3f ms; " % sc + versus(sc, sa))
        del layers, autograd, chunk, module
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
