#!/usr/bin/env python3
"""Times of what OM-LSTM adds, each against its yardstick on the same inputs and the same device:
(a) ebc_observe_wide_sorted (one kernel: the rows by decreasing distance, the maps built from the rows in that order)
    against the composition it replaces (ebc_observe twice, ebc_row_counts, a torch sort of the distance column, two
    gathers, ebc_occupancy_rows and a torch.cat), 4096 envs of 5 and of 10 rows;
(b) a decision batch of DeviceSarlPolicy over LstmValueNet with maps (rows 61 wide) and without (rows 13 wide), both value
    networks;
(c) ebc_lstm_grad on 61-wide rows against torch autograd of LstmModule, 100 and 4096 states of 5 and 10 rows, both value
    networks; ebc_lstm_net_grad_max_rows of each network is printed.

    python3 tools/om_lstm_bench.py [--blocks 7] [--reps 20] [--out profiles/om_lstm.txt]

The method is tools/om_train_bench.py's: warm-up first, then the median over `--blocks` blocks of `--reps` back-to-back
calls, by a pair of events on the stream and by the host's clock around the block with a synchronize at its end."""
import argparse
import configparser
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _capi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.lstm_rl import LstmModule, LstmValueNet
    from ebcsim.lstm_train import LstmTrainer
    from ebcsim.occupancy import OccupancySpec, observe_wide_sorted_composed
    from ebcsim.sarl import DeviceSarlPolicy
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn, reps=None):
        reps = args.reps if reps is None else reps
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

    dev = torch.device("cuda:0")
    say("# tools/om_lstm_bench.py --blocks %d --reps %d --envs %d: ms per call, median (min .. max) of the blocks by stream events, and "
        "the host clock's median; maps 4 x 4 cells of 1 m, 3 channels (W = 48, rows 13 + 48 = 61 wide); %s; library %s"
        % (args.blocks, args.reps, args.envs, torch.cuda.get_device_name(0), os.path.basename(_capi.LIB_PATH)))
    om = OccupancySpec(4, 1.0, 3)
    DIMS = dict(mlp2=[150, 100, 100, 1], hidden=50, mlp1=[150, 100, 100, 50])

    def module(width, two):
        torch.manual_seed(11)
        return LstmModule(width, 6, DIMS["mlp2"], DIMS["hidden"], DIMS["mlp1"] if two else None)

    def env_of(adults, E):
        cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
        cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"))
        cfg.set("sim", "adult_num", str(adults))
        pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_om_lstm.config"))
        params = ebc_config.params_from_config(cfg, pol, policy="om_lstm_rl")
        sc = ebc_scene.SceneConfig.from_config(cfg)
        gen = ebc_scene.gen_struct(sc, "train")
        env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
        env.use_torch_stream()
        seed0 = ebc_scene.COUNTER_OFFSET["train"]
        env.generate_reset(gen, seed0)
        return env, ebc_actions.build_action_space(sc.robot.v_pref)

    # ---- (a) and (b)
    for adults in (5, 10):
        env, space = env_of(adults, args.envs)
        E, R, T = env.E, env.R, env.T
        out = torch.empty((E, R, T + om.width), dtype=torch.float32, device=dev)
        n = torch.empty((E,), dtype=torch.int64, device=dev)
        env.observe_wide_sorted_device(out, om, n)
        ref = observe_wide_sorted_composed(env, om)
        plain = torch.empty_like(out)
        env.observe_wide_device(plain, om)
        torch.cuda.synchronize()
        say("(a) E %d R %2d T %d: ebc_observe_wide_sorted equals the composition: %s; rows moved in %d of %d envs" % (
            E, R, T, bool(torch.equal(out, ref)), int((out[:, :, :T] != plain[:, :, :T]).any(2).any(1).sum()), E))
        k = timed(lambda: env.observe_wide_sorted_device(out, om, n))
        c = timed(lambda: observe_wide_sorted_composed(env, om, n_rows=n))
        u = timed(lambda: env.observe_wide_device(plain, om, n))
        say("(a) E %d R %2d  ebc_observe_wide_sorted (one kernel)                                             : %8.4f ms (%.4f .. %.4f), host clock %.4f ms" % ((E, R) + k))
        say("(a) E %d R %2d  ebc_observe x 2, ebc_row_counts, torch sort, 2 gathers, ebc_occupancy_rows, cat  : %8.4f ms (%.4f .. %.4f), host clock %.4f ms" % ((E, R) + c))
        say("(a) E %d R %2d  ebc_observe_wide (the env's order, for scale)                                    : %8.4f ms (%.4f .. %.4f), host clock %.4f ms" % ((E, R) + u))
        say("(a) E %d R %2d  composition / kernel: %.2f x by events, %.2f x by the host clock" % (E, R, c[0] / k[0], c[3] / k[3]))
        for two in (True, False):
            name = "ValueNetwork2 (mlp1)" if two else "ValueNetwork1 (no mlp1)"
            wide_pol = DeviceSarlPolicy(LstmValueNet(module(T + om.width, two).state_dict(), device=dev), space, 0.9, om=om)
            bare_pol = DeviceSarlPolicy(LstmValueNet(module(T, two).state_dict(), device=dev), space, 0.9)
            reps = max(2, args.reps // 4)
            w = timed(lambda: wide_pol.decide(env), reps)
            b = timed(lambda: bare_pol.decide(env), reps)
            say("(b) E %d R %2d %-24s decision batch with maps (rows 61 wide)   : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((E, R, name) + w))
            say("(b) E %d R %2d %-24s decision batch without maps (rows 13 wide): %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((E, R, name) + b))
            say("(b) E %d R %2d %-24s with maps / without: %.3f x by events, %.3f x by the host clock" % (E, R, name, w[0] / b[0], w[3] / b[3]))
        env.synchronize()
        env.close()

    # ---- (c)
    width = 13 + om.width
    for two in (True, False):
        name = "ValueNetwork2" if two else "ValueNetwork1"
        sd = module(width, two).state_dict()
        native = LstmTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=True)
        auto = LstmTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=False)
        m = module(width, two).to(dev)
        m.load_state_dict(sd)
        max_rows = native.net.grad_max_rows()
        say("# %s, rows %d wide: ebc_lstm_net_grad_max_rows = %d" % (name, width, max_rows))
        for B, R in ((100, 5), (100, 10), (4096, 5), (4096, 10)):
            if R > max_rows:
                say("(c) %s B %4d R %2d: more rows than ebc_lstm_grad takes for this network (%d); not timed" % (name, B, R, max_rows))
                continue
            g = torch.Generator(device=dev).manual_seed(1000 * B + R + int(two))
            rows = torch.randn((B, R, width), generator=g, device=dev)
            rows[:, :, 13:] = (rows[:, :, 13:] > 0.8).float()  # maps: mostly empty cells
            target = 0.5 * torch.randn((B,), generator=g, device=dev)
            scale = 2.0 / B

            def bare():
                for p_ in m.parameters():
                    p_.grad = None
                torch.nn.functional.mse_loss(m(rows).squeeze(1), target).backward()

            def grad(tr):
                return tr.loss_and_grad(rows, target, grad_scale=scale)
            ln, cn = grad(native)
            la, ca = grad(auto)
            torch.cuda.synchronize()
            gn, ga = native.flat.grad, auto.flat.grad
            tag = (name, B, R)
            say("(c) %s B %4d R %2d: count %d / %d, loss_sum %.9g / %.9g, largest |kernel - autograd| of the gradient %.3g (largest entry %.3g)"
                % (tag + (int(cn), int(ca), float(ln), float(la), float((gn - ga).abs().max()), float(ga.abs().max()))))
            k = timed(lambda: grad(native))
            a = timed(bare)
            say("(c) %s B %4d R %2d  ebc_lstm_grad on 61-wide rows              : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % (tag + k))
            say("(c) %s B %4d R %2d  torch autograd of LstmModule                : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % (tag + a))
            say("(c) %s B %4d R %2d  autograd / kernel: %.2f x by events, %.2f x by the host clock" % (tag + (a[0] / k[0], a[3] / k[3])))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
