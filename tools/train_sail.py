#!/usr/bin/env python3
"""Train the SAIL network by imitation of the ORCA robot on the device and score it: demonstrations from `--envs` envs on
device-generated train scenes (ebcsim.sail_train.collect_sail_demos), `--epochs` passes of minibatch regression with the
fused gradient kernel (ebc_sail_grad) and Adam, the weights saved in the reference's ExtendedNetwork layout, then the
evaluation tools/evaluate.py --policy sail runs on the test cases, with the reference's metrics.

    python3 tools/train_sail.py --env-config ENV_WITH_ADULT_NUM_ROWS --device-scenes [--envs 1024] [--demo-steps 120]
                                [--epochs 50] [--batch-size 1024] [--lr 1e-3] [--cases 500] [--out sail_model.pth]
                                [--dagger-rounds N] [--dagger-steps 60] [--dagger-epochs 10] [--beta0 0.5] [--beta-decay 0.5]
                                [--capacity 1000000] [--demo-steps-per-call K [--demo-one-launch]]

--demo-steps-per-call K collects the demonstrations in windows of K steps per call (ebc_step_k_world, which records the
robot's state and the world-frame rows on the device) instead of five calls per step; --demo-one-launch runs each window
as one kernel launch.  The demonstrations are the same bytes.

--dagger-rounds N > 0 continues with N rounds of DAgger (ebcsim.sail_train.dagger): the network drives the training envs
(mixed with the demonstrator with probability beta0 * beta_decay^(i - 1)), the demonstrator labels every state it
visits in one ebc_sail_dagger_k call per round, and the fit runs on the aggregate.  The closing evaluation then runs after
every round (round 0 = the behaviour-cloning baseline of the same run) and the JSON line gains the per-round list.

The env config's scenes must have exactly adult_num rows each (the network takes no other count)."""
import argparse
import configparser
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--env-config", required=True)
    ap.add_argument("--policy-config", default=os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    ap.add_argument("--device-scenes", action="store_true", help="generate the scenes on the device (required: the only form built)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--demo-steps", type=int, default=120)
    ap.add_argument("--demo-steps-per-call", type=int, default=None, metavar="K",
                    help="collect the demonstrations K steps per call (ebc_step_k_world); default: the per-step loop")
    ap.add_argument("--demo-one-launch", action="store_true", help="each of those calls as one kernel launch")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--safety-space", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--cases", type=int, default=500, help="test cases of the closing evaluation")
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--autograd", action="store_true", help="torch autograd instead of the kernel (the comparison path)")
    ap.add_argument("--out", default="sail_model.pth")
    ap.add_argument("--dagger-rounds", type=int, default=0, help="rounds of DAgger after the behaviour cloning (0: none)")
    ap.add_argument("--dagger-steps", type=int, default=60, help="steps of every env per DAgger round")
    ap.add_argument("--dagger-epochs", type=int, default=10, help="passes over the aggregate per DAgger round")
    ap.add_argument("--beta0", type=float, default=0.5, help="probability that a step of round 1 executes the expert's action")
    ap.add_argument("--beta-decay", type=float, default=0.5, help="factor on that probability from round to round")
    ap.add_argument("--capacity", type=int, default=1000000, help="samples the aggregate keeps (the oldest leave first)")
    args = ap.parse_args()
    if args.demo_one_launch and args.demo_steps_per_call is None:
        ap.error("--demo-one-launch needs --demo-steps-per-call")
    if not args.device_scenes:
        ap.error("--device-scenes is required: demonstrations restart from a pool of device-generated scenes")
    import torch
    from ebcsim import _abi, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailModule, SailNet
    from ebcsim.sail_train import SailTrainer, collect_sail_demos, dagger, fit
    from ebcsim.train import evaluate
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(args.env_config)
    pol.read(args.policy_config)
    params = ebc_config.params_from_config(cfg, pol, policy="sail")
    humans = ebc_config.human_policies_from_config(cfg)  # the env config's, per entity type
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "train")
    N = sum(gen.count)
    if ebc_scene.max_static_rows(sc):
        ap.error("the env config has static rows: SAIL takes exactly adult_num rows per scene")
    E = args.envs
    test = ebc_scene.gen_struct(sc, "test")

    def evaluate_saved():
        """what tools/evaluate.py --policy sail --device-scenes runs, on the file just saved -> the metrics, printed"""
        env = BatchedEnv(params, args.cases, sum(test.count), 0)
        env.generate_reset(test, ebc_scene.COUNTER_OFFSET["test"])
        env.synchronize()
        env.use_torch_stream()
        env.configure_humans(*humans)
        policy = DeviceSailPolicy(SailNet.load(args.out, device="cuda:0"))
        m = evaluate(env, lambda e: policy.decide(e)[0], args.gamma)
        torch.cuda.synchronize()
        env.close()
        print("TEST  has success rate: %.2f, collision rate adult / bicycle / child / obstacle: %.2f / %.2f / %.2f / %.4f, "
              "timeout: %d, nav time: %.2f, total reward: %.4f" % (
                  m["success_rate"], m["collision_rate_adult"], m["collision_rate_bicycle"], m["collision_rate_child"],
                  m["collision_rate_obstacle"], m["timeout"], m["avg_nav_time"], m["total_reward:"]))
        print("Frequency of being in danger: %.2f and average min separate distance in danger: %.2f" % (
            m["Frequency of being in danger"] or 0.0, m["average min separate distance in danger"]))
        return {k: v for k, v in m.items() if not isinstance(v, list)}

    env = BatchedEnv(params, E, N, 0)
    env.use_torch_stream()
    env.configure_humans(*humans)
    seed0 = ebc_scene.COUNTER_OFFSET["train"]
    env.generate_reset(gen, seed0)
    env.generate_pool(gen, seed0 + E, 4 * E)
    if args.dagger_rounds > 0:
        torch.manual_seed(args.seed)
        trainer = SailTrainer(SailModule(N), device="cuda:0", optimizer="adam", lr=args.lr, native=not args.autograd)
        per_round = []

        def on_round(i, info):
            torch.cuda.synchronize()
            trainer.save(args.out)
            print("round %d: beta %.3f, %d episodes ended in the window%s, %d samples kept, aggregate %d; mean squared error "
                  "first %.6f, last %.6f; saved %s" % (
                      i, info["beta"], info["episodes"],
                      "" if i == 0 else " (%d success, %d collision, %d timeout)" % (info["success"], info["collision"], info["timeout"]),
                      info["samples"], info["aggregate"], info["losses"][0], info["losses"][-1], args.out))
            row = {k: v for k, v in info.items() if k != "losses"}
            row.update(losses=[info["losses"][0], info["losses"][-1]], metrics=evaluate_saved())
            per_round.append(row)

        t0 = time.perf_counter()
        dagger(env, trainer, args.dagger_rounds, args.demo_steps, args.dagger_steps, args.epochs, args.dagger_epochs, args.batch_size,
               beta0=args.beta0, beta_decay=args.beta_decay, capacity=args.capacity,
               generator=torch.Generator(device="cuda:0").manual_seed(args.seed), safety_space=args.safety_space, on_round=on_round,
               demo_steps_per_call=args.demo_steps_per_call, demo_one_launch=args.demo_one_launch)
        torch.cuda.synchronize()
        print("%d rounds of DAgger after the behaviour cloning in %.2f s (the evaluations included)" % (args.dagger_rounds, time.perf_counter() - t0))
        env.close()
        print(json.dumps({"envs": E, "demo_steps": args.demo_steps, "kept": per_round[0]["samples"], "epochs": args.epochs,
                          "losses": per_round[0]["losses"], "cases": args.cases, "metrics": per_round[-1]["metrics"],
                          "dagger": {"rounds": args.dagger_rounds, "steps": args.dagger_steps, "epochs": args.dagger_epochs,
                                     "beta0": args.beta0, "beta_decay": args.beta_decay, "capacity": args.capacity},
                          "rounds": per_round}))
        return
    t0 = time.perf_counter()
    demos = collect_sail_demos(env, args.demo_steps, args.safety_space, steps_per_call=args.demo_steps_per_call,
                               one_launch=args.demo_one_launch)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print("demonstrations: %d envs x %d steps, %d episodes ended, %d steps kept (ReachGoal episodes) in %.2f s"
          % (E, args.demo_steps, demos["episodes"], demos["steps"], t1 - t0))
    env.close()
    torch.manual_seed(args.seed)
    trainer = SailTrainer(SailModule(N), device="cuda:0", optimizer="adam", lr=args.lr, native=not args.autograd)
    losses = fit(trainer, demos, args.epochs, args.batch_size, generator=torch.Generator(device="cuda:0").manual_seed(args.seed))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print("fit: %d epochs of %d batches (%s) in %.2f s; mean squared error per epoch: first %.6f, last %.6f"
          % (args.epochs, -(-demos["steps"] // args.batch_size), "torch autograd" if args.autograd else "ebc_sail_grad", t2 - t1,
             losses[0], losses[-1]))
    trainer.save(args.out)
    print("saved %s" % args.out)
    m = evaluate_saved()
    print(json.dumps({"envs": E, "demo_steps": args.demo_steps, "kept": demos["steps"], "epochs": args.epochs, "losses": [losses[0], losses[-1]],
                      "cases": args.cases, "metrics": m}))


if __name__ == "__main__":
    main()
