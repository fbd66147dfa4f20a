#!/usr/bin/env python3
"""Train the CADRL value network on the device and score it: the schedule of rl/train.py (imitation learning from the ORCA
robot, then epsilon-greedy RL rounds with a target network) on `--envs` envs of device-generated train scenes
(ebcsim.cadrl_train.run_cadrl_training), the gradient by the fused kernel (ebc_cadrl_grad), the weights saved in the
reference's ValueNetwork layout, then the evaluation tools/evaluate.py --policy cadrl --weights runs on the test cases,
with the reference's metrics, after imitation learning and after RL.

    python3 tools/train_cadrl.py --env-config eb-cadrl_amd/configs/cadrl_one_human.config \
        --policy-config eb-cadrl_amd/configs/policy_plain.config --device-scenes [--envs 256] [--il-steps 200] [--il-epochs 50]
        [--iterations 200] [--steps-per-iteration 4] [--train-batches 100] [--batch-size 100] [--cases 500] [--out cadrl_model.pth]

The tool's defaults are a SHORT schedule, not the reference's: 200 RL rounds with epsilon decayed over 150 of them and the
target network refreshed every 10 (--epsilon-decay 150, --target-update-interval 10), where run_cadrl_training and the
reference's train.config use 4000 and 50 for runs of 10 000 rounds; pass those for a run of that length.

A reward, value target or loss that is not finite stops the run with an error before an optimizer step sees it; --out is
written only by a run that ended.

The reference trains CADRL on one-human scenes (its transform asserts a single other agent); with more rows per state the
value is the minimum over the rows and the gradient goes through the minimal row, this project's batched extension."""
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
    ap.add_argument("--policy-config", default=os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_plain.config"))
    ap.add_argument("--device-scenes", action="store_true", help="generate the scenes on the device (required: the only form built)")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--mlp-dims", default="150, 100, 100, 1", help="[cadrl] mlp_dims when the policy config has no [cadrl] section")
    ap.add_argument("--il-steps", type=int, default=200)
    ap.add_argument("--il-epochs", type=int, default=50)
    ap.add_argument("--il-lr", type=float, default=0.01)
    ap.add_argument("--rl-lr", type=float, default=0.001)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--steps-per-iteration", type=int, default=4)
    ap.add_argument("--train-batches", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--epsilon-start", type=float, default=0.5)
    ap.add_argument("--epsilon-end", type=float, default=0.1)
    ap.add_argument("--epsilon-decay", type=int, default=150)
    ap.add_argument("--target-update-interval", type=int, default=10)
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "adam"])
    ap.add_argument("--safety-space", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--cases", type=int, default=500, help="test cases of the evaluations")
    ap.add_argument("--gamma", type=float, default=None, help="default: [rl] gamma of the policy config")
    ap.add_argument("--autograd", action="store_true", help="torch autograd instead of the kernel (the comparison path)")
    ap.add_argument("--out", default="cadrl_model.pth")
    args = ap.parse_args()
    if not args.device_scenes:
        ap.error("--device-scenes is required: the rollouts restart from a pool of device-generated scenes")
    if args.il_steps < 1:
        ap.error("--il-steps >= 1: the schedule starts with imitation learning, whose model is scored first")
    import torch
    from ebcsim import _abi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.cadrl import CadrlModule, CadrlValueNet, DeviceCadrlPolicy
    from ebcsim.cadrl_train import CadrlTrainer, run_cadrl_training
    from ebcsim.train import evaluate
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(args.env_config)
    pol.read(args.policy_config)
    params = ebc_config.params_from_config(cfg, pol, policy="cadrl")
    humans = ebc_config.human_policies_from_config(cfg)  # the env config's, per entity type
    gamma = args.gamma if args.gamma is not None else pol.getfloat("rl", "gamma", fallback=0.9)
    dims = [int(x) for x in pol.get("cadrl", "mlp_dims", fallback=args.mlp_dims).split(",")]
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen, test = ebc_scene.gen_struct(sc, "train"), ebc_scene.gen_struct(sc, "test")
    S = ebc_scene.max_static_rows(sc)
    space = ebc_actions.build_action_space(sc.robot.v_pref)
    out_dir = os.path.dirname(os.path.abspath(args.out))

    def evaluate_saved(path, label):
        """what tools/evaluate.py --policy cadrl --weights PATH --device-scenes runs -> the metrics, printed"""
        env = BatchedEnv(params, args.cases, sum(test.count), S)
        env.generate_reset(test, ebc_scene.COUNTER_OFFSET["test"])
        env.synchronize()
        env.use_torch_stream()
        env.configure_humans(*humans)
        policy = DeviceCadrlPolicy(CadrlValueNet.load(path, device="cuda:0"), space, gamma)
        m = evaluate(env, lambda e: policy.decide(e)[0], gamma, human_policy=_abi.HUMAN_CACHED)
        torch.cuda.synchronize()
        env.close()
        print("TEST  %s has success rate: %.2f, collision rate adult / bicycle / child / obstacle: %.2f / %.2f / %.2f / %.4f, "
              "timeout: %d, nav time: %.2f, total reward: %.4f" % (
                  label, m["success_rate"], m["collision_rate_adult"], m["collision_rate_bicycle"], m["collision_rate_child"],
                  m["collision_rate_obstacle"], m["timeout"], m["avg_nav_time"], m["total_reward:"]))
        print("Frequency of being in danger: %.2f and average min separate distance in danger: %.2f" % (
            m["Frequency of being in danger"] or 0.0, m["average min separate distance in danger"]))
        return {k: v for k, v in m.items() if not isinstance(v, list)}

    E = args.envs
    env = BatchedEnv(params, E, sum(gen.count), S)
    env.use_torch_stream()
    env.configure_humans(*humans)
    seed0 = ebc_scene.COUNTER_OFFSET["train"]
    env.generate_reset(gen, seed0)
    env.generate_pool(gen, seed0 + E, 8 * E)
    torch.manual_seed(args.seed)
    trainer = CadrlTrainer(CadrlModule(env.T, dims), device="cuda:0", optimizer=args.optimizer, lr=args.il_lr, native=not args.autograd)
    g = torch.Generator(device="cuda:0").manual_seed(args.seed)
    common = dict(il_learning_rate=args.il_lr, il_safety_space=args.safety_space, rl_learning_rate=args.rl_lr, steps_per_iteration=args.steps_per_iteration,
                  train_batches=args.train_batches, batch_size=args.batch_size, capacity=args.capacity, epsilon_start=args.epsilon_start,
                  epsilon_end=args.epsilon_end, epsilon_decay=args.epsilon_decay, target_update_interval=args.target_update_interval, generator=g,
                  output_dir=out_dir, log=lambda line: print(line, flush=True) if not line.startswith("iteration") or int(line.split()[1][:-1]) % 10 == 0 else None)
    t0 = time.perf_counter()
    mark = {}

    def after_il(h):
        torch.cuda.synchronize()
        mark["il_s"] = time.perf_counter() - t0
        print("imitation learning (%s): %d envs x %d steps, %d states of %d episodes, %d epochs in %.2f s"
              % ("torch autograd" if args.autograd else "ebc_cadrl_grad", E, args.il_steps, h["il_stored"], h["il_episodes"], args.il_epochs, mark["il_s"]))
        mark["after_il"] = evaluate_saved(os.path.join(out_dir, "il_model.pth"), "after imitation learning")
        mark["t_rl"] = time.perf_counter()

    hist = run_cadrl_training(env, trainer, space, gamma, il_steps=args.il_steps, il_epochs=args.il_epochs, train_iterations=args.iterations,
                              after_il=after_il, **common)
    torch.cuda.synchronize()
    rl_s = time.perf_counter() - mark["t_rl"]
    print("RL: %d rounds of %d decisions per env and %d optimizer steps of batch %d in %.2f s; loss first %.3e, last %.3e; replay memory %d"
          % (args.iterations, args.steps_per_iteration, args.train_batches, args.batch_size, rl_s,
             hist["rl_loss"][0] if hist["rl_loss"] else float("nan"), hist["rl_loss"][-1] if hist["rl_loss"] else float("nan"), hist["memory"]))
    env.close()
    trainer.save(args.out)
    print("saved %s" % args.out)
    after_rl = evaluate_saved(args.out, "after RL")
    print(json.dumps({"envs": E, "il_steps": args.il_steps, "il_epochs": args.il_epochs, "il_stored": hist["il_stored"], "il_loss": hist["il_loss"],
                      "iterations": args.iterations, "rl_loss": [hist["rl_loss"][0], hist["rl_loss"][-1]] if hist["rl_loss"] else [],
                      "il_s": mark["il_s"], "rl_s": rl_s, "cases": args.cases, "after_il": mark["after_il"], "after_rl": after_rl}))


if __name__ == "__main__":
    main()
