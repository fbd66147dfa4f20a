#!/usr/bin/env python3
"""Times of what training OM-SARL adds, each against its yardstick on the same inputs and the same device:
(a) ebc_observe_wide against the four-call composition it replaces (ebc_observe twice, ebc_row_counts, ebc_occupancy_rows
    and a torch.cat), 4096 envs of 5 and of 10 rows;
(b) ebc_sarl_grad on the wide network at T + W = 61 and 65, R = 5 and 10, B = 100 and 4096, against torch autograd of the
    wide SarlModule;
(c) a full trainer step, SarlTrainer native against SarlTrainer autograd;
(d) an imitation window of K steps with maps (ebc_step_k_om) and without (ebc_step_k), and the composition the window
    with maps replaces (per step the four calls, then ebc_step_k of one step).

    python3 tools/om_train_bench.py [--blocks 7] [--reps 20] [--out profiles/om_train.txt]

The method is tools/sarl_train_bench.py's: warm-up first, then the median over `--blocks` blocks of `--reps` back-to-back
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

UNITS = dict(mlp1_dims=[150, 100], mlp2_dims=[100, 50], mlp3_dims=[150, 100, 100, 1], attention_dims=[100, 100, 1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--window", type=int, default=20, help="steps of the imitation window of (d)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    from ebcsim import _abi, _capi, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.occupancy import OccupancySpec, observe_wide_composed
    from ebcsim.sarl_train import SarlTrainer
    from ebcsim.train import SarlModule
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
    say("# tools/om_train_bench.py --blocks %d --reps %d --envs %d --window %d: ms per call, median (min .. max) of the blocks by stream "
        "events, and the host clock's median; maps 4 x 4 cells of 1 m, 3 channels (W = 48); %s; library %s"
        % (args.blocks, args.reps, args.envs, args.window, torch.cuda.get_device_name(0), os.path.basename(_capi.LIB_PATH)))
    om = OccupancySpec(4, 1.0, 3)

    def env_of(adults, policy_config, E):
        cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
        cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"))
        cfg.set("sim", "adult_num", str(adults))
        pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", policy_config))
        params = ebc_config.params_from_config(cfg, pol)
        sc = ebc_scene.SceneConfig.from_config(cfg)
        gen = ebc_scene.gen_struct(sc, "train")
        env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
        env.use_torch_stream()
        seed0 = ebc_scene.COUNTER_OFFSET["train"]
        env.generate_reset(gen, seed0)
        env.generate_pool(gen, seed0 + E, 2 * E)
        return env

    # ---- (a) and (d)
    for adults in (5, 10):
        env = env_of(adults, "policy_om.config", args.envs)
        E, R, T = env.E, env.R, env.T
        out = torch.empty((E, R, T + om.width), dtype=torch.float32, device=dev)
        ref = torch.empty_like(out)
        n = torch.empty((E,), dtype=torch.int64, device=dev)
        env.observe_wide_device(out, om, n)
        observe_wide_composed(env, om, out=ref)
        torch.cuda.synchronize()
        say("(a) E %d R %2d T %d: ebc_observe_wide equals the composition: %s" % (E, R, T, bool(torch.equal(out, ref))))
        k = timed(lambda: env.observe_wide_device(out, om, n))
        c = timed(lambda: observe_wide_composed(env, om, out=ref, n_rows=n))
        say("(a) E %d R %2d  ebc_observe_wide (one kernel)                                        : %8.4f ms (%.4f .. %.4f), host clock %.4f ms" % ((E, R) + k))
        say("(a) E %d R %2d  ebc_observe x 2, ebc_row_counts, ebc_occupancy_rows, torch.cat, copy : %8.4f ms (%.4f .. %.4f), host clock %.4f ms" % ((E, R) + c))
        say("(a) E %d R %2d  composition / kernel: %.2f x by events, %.2f x by the host clock" % (E, R, c[0] / k[0], c[3] / k[3]))
        K = args.window
        kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, flags=_abi.FLAG_AUTO_RESET, robot_safety_space=0.15)
        keys = ("reward", "done", "info")
        plain = env.alloc_step_k_outputs(K, keys + ("state_rotated",))
        wide = env.alloc_step_k_outputs(K, keys + ("state_wide",), om=om)
        one = env.alloc_step_k_outputs(1, keys)

        def window_composed():
            for k_ in range(K):
                observe_wide_composed(env, om, out=wide["state_wide"][k_])
                env.step_k_device(one, 1, **kw)
        reps = max(2, args.reps // 4)
        p = timed(lambda: env.step_k_device(plain, K, **kw), reps)
        w = timed(lambda: env.step_k_device(wide, K, om=om, **kw), reps)
        cw = timed(window_composed, reps)
        say("(d) E %d R %2d K %d  ebc_step_k, rotated states (no maps)                 : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((E, R, K) + p))
        say("(d) E %d R %2d K %d  ebc_step_k_om, wide states                           : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((E, R, K) + w))
        say("(d) E %d R %2d K %d  per step the four-call composition + ebc_step_k(1)   : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % ((E, R, K) + cw))
        say("(d) E %d R %2d K %d  with maps / without: %.3f x by events; composition / ebc_step_k_om: %.2f x by events, %.2f x by the host clock"
            % (E, R, K, w[0] / p[0], cw[0] / w[0], cw[3] / w[3]))
        env.synchronize()
        env.close()

    # ---- (b) and (c)
    for T in (13, 17):
        torch.manual_seed(11)
        sd = SarlModule(T + om.width, **UNITS).state_dict()
        native = SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=True, om_width=om.width)
        auto = SarlTrainer(sd, device=dev, optimizer="sgd", lr=1e-3, native=False, om_width=om.width)
        module = SarlModule(T + om.width, **UNITS).to(dev)
        module.load_state_dict(sd)
        say("# T + W = %d: ebc_sarl_net_grad_max_rows = %d" % (T + om.width, native.net.grad_max_rows()))
        for B, R in ((100, 5), (100, 10), (4096, 5), (4096, 10)):
            g = torch.Generator(device=dev).manual_seed(1000 * B + R + T)
            rows = torch.randn((B, R, T + om.width), generator=g, device=dev)
            rows[:, :, T:] = (rows[:, :, T:] > 0.8).float()  # maps: mostly empty cells
            target = 0.5 * torch.randn((B,), generator=g, device=dev)
            scale = 2.0 / B

            def bare():
                for p_ in module.parameters():
                    p_.grad = None
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
            tag = (T + om.width, B, R)
            say("(b) T+W %d B %4d R %2d: count %d / %d, loss_sum %.9g / %.9g, largest |kernel - autograd| of the gradient %.3g (largest entry %.3g)"
                % (tag + (int(cn), int(ca), float(ln), float(la), float((gn - ga).abs().max()), float(ga.abs().max()))))
            k = timed(lambda: grad(native))
            a = timed(bare)
            say("(b) T+W %d B %4d R %2d  ebc_sarl_grad on wide rows                      : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % (tag + k))
            say("(b) T+W %d B %4d R %2d  torch autograd of the wide SarlModule           : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % (tag + a))
            say("(b) T+W %d B %4d R %2d  autograd / kernel: %.2f x by events, %.2f x by the host clock" % (tag + (a[0] / k[0], a[3] / k[3])))
            ks = timed(lambda: step(native))
            as_ = timed(lambda: step(auto))
            say("(c) T+W %d B %4d R %2d  full step, SarlTrainer native                   : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % (tag + ks))
            say("(c) T+W %d B %4d R %2d  full step, SarlTrainer autograd                 : %8.3f ms (%.3f .. %.3f), host clock %.3f ms" % (tag + as_))
            say("(c) T+W %d B %4d R %2d  autograd step / native step: %.2f x by events, %.2f x by the host clock" % (tag + (as_[0] / ks[0], as_[3] / ks[3])))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
