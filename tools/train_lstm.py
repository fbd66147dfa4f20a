#!/usr/bin/env python3
"""Train an LSTM-RL value network on the device and score it: the schedule of rl/train.py (imitation learning from the ORCA
robot, then epsilon-greedy RL rounds with a target network, the RL states sorted by decreasing distance as LstmRL.predict
leaves them) on `--envs` envs of device-generated train scenes (ebcsim.lstm_train.run_lstm_training), the gradient by the
fused kernel (ebc_lstm_grad) or, with --autograd, by torch autograd of LstmModule, the weights saved in the reference's
ValueNetwork1 / ValueNetwork2 layout (loads there with strict=True), then the evaluation tools/evaluate.py --policy lstm_rl
--weights runs on the test cases, with the reference's metrics, after imitation learning and after RL.

    python3 tools/train_lstm.py --env-config eb-cadrl_amd/configs/sarl_a5.config \
        --policy-config eb-cadrl_amd/configs/policy_lstm.config --device-scenes [--interaction-module true|false]
        [--envs 256] [--il-steps 200] [--il-epochs 50] [--iterations 200] [--steps-per-iteration 4] [--train-batches 100]
        [--batch-size 100] [--cases 500] [--weights start.pth] [--autograd] [--out lstm_model.pth]

--interaction-module overrides [lstm_rl] with_interaction_module of the policy config: true is ValueNetwork2 (rows -> mlp1 ->
LSTM -> mlp), false ValueNetwork1 (rows -> LSTM -> mlp).

The tool's defaults are a SHORT schedule, not the reference's: 200 RL rounds with epsilon decayed over 150 of them and the
target network refreshed every 10, where run_lstm_training and the reference's train.config use 4000 and 50 for runs of
10 000 rounds; pass those for a run of that length.

OM-LSTM: with [lstm_rl] with_om = true in the policy config (eb-cadrl_amd/configs/policy_om_lstm.config: [om] 4 / 1 / 3) the
network's rows are 13 + cell_num^2 * om_channel_size = 61 wide and the schedule is run_lstm_training(..., om=spec): the
imitation window stores the wide states in the env's order (ebc_step_k_om), the RL rounds the sorted wide state — the rows
by decreasing distance with the maps built from the rows in THAT order, one kernel (ebc_observe_wide_sorted) — and
DeviceSarlPolicy(om=spec) decides and scores.  The saved file loads into the reference's ValueNetwork1(61, ...) /
ValueNetwork2(61, ...) with strict=True; tools/evaluate.py --policy lstm_rl --policy-config that config --weights scores it.

A reward, value target or loss that is not finite stops the run with an error before an optimizer step sees it; --out is
written only by a run that ended."""
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
    ap.add_argument("--policy-config", default=os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_lstm.config"))
    ap.add_argument("--device-scenes", action="store_true", help="generate the scenes on the device (required: the only form built)")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--weights", default=None, help="a state_dict in the reference's layout to start from (default: torch's initialisation)")
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
    ap.add_argument("--states-per-pass", default=None, choices=["auto", "1", "2", "4"],
                    help="the kernel runs a chunk's 4 states that many at a time, which takes more rows per state (the same bytes); "
                         "auto: the largest that holds the scene's rows.  Default: the whole chunk at once")
    ap.add_argument("--interaction-module", default=None, choices=["true", "false"],
                    help="ValueNetwork2 (true) or ValueNetwork1 (false); default: [lstm_rl] with_interaction_module of the policy config")
    ap.add_argument("--out", default="lstm_model.pth")
    args = ap.parse_args()
    if not args.device_scenes:
        ap.error("--device-scenes is required: the rollouts restart from a pool of device-generated scenes")
    if args.il_steps < 1:
        ap.error("--il-steps >= 1: the schedule starts with imitation learning, whose model is scored first")
    import torch
    from ebcsim import _abi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.lstm_rl import LstmModule, LstmValueNet
    from ebcsim.lstm_train import LstmTrainer, run_lstm_training
    from ebcsim.sarl import DeviceSarlPolicy
    from ebcsim.train import evaluate
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(args.env_config)
    pol.read(args.policy_config)
    params = ebc_config.params_from_config(cfg, pol)
    humans = ebc_config.human_policies_from_config(cfg)  # the env config's, per entity type
    gamma = args.gamma if args.gamma is not None else pol.getfloat("rl", "gamma", fallback=0.9)
    dims = {k: [int(x) for x in pol.get("lstm_rl", k, fallback=d).split(",")] for k, d in (
        ("mlp1_dims", "150, 100, 100, 50"), ("mlp2_dims", "150, 100, 100, 1"))}
    hidden = pol.getint("lstm_rl", "global_state_dim", fallback=50)
    two = pol.getboolean("lstm_rl", "with_interaction_module", fallback=True) if args.interaction_module is None else args.interaction_module == "true"
    from ebcsim.occupancy import OccupancySpec
    om = OccupancySpec.from_config(pol, section="lstm_rl")  # None without [lstm_rl] with_om = true
    kw_om = {} if om is None else {"om": om}
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen, test = ebc_scene.gen_struct(sc, "train"), ebc_scene.gen_struct(sc, "test")
    S = ebc_scene.max_static_rows(sc)
    space = ebc_actions.build_action_space(sc.robot.v_pref)
    out_dir = os.path.dirname(os.path.abspath(args.out))

    def evaluate_saved(path, label):
        """what tools/evaluate.py --policy lstm_rl --weights PATH --device-scenes runs -> the metrics, printed"""
        env = BatchedEnv(params, args.cases, sum(test.count), S)
        env.generate_reset(test, ebc_scene.COUNTER_OFFSET["test"])
        env.synchronize()
        env.use_torch_stream()
        env.configure_humans(*humans)
        policy = DeviceSarlPolicy(LstmValueNet.load(path, device="cuda:0"), space, gamma, **kw_om)
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
    width = env.T + (om.width if om is not None else 0)
    if width > 64:
        ap.error("rows of %d + %d map columns = %d: the LSTM kernels take rows up to 64 wide" % (env.T, om.width, width))
    start = LstmModule(width, 6, dims["mlp2_dims"], hidden, dims["mlp1_dims"] if two else None)
    if args.weights:
        start.load_state_dict(torch.load(args.weights, map_location="cpu"), strict=True)
    spp = args.states_per_pass if args.states_per_pass in (None, "auto") else int(args.states_per_pass)
    trainer = LstmTrainer(start, device="cuda:0", optimizer=args.optimizer, lr=args.il_lr, native=not args.autograd, states_per_pass=spp)
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
        print("imitation learning (%s, rows %d wide): %d envs x %d steps, %d states of %d episodes, %d epochs in %.2f s"
              % ("torch autograd" if args.autograd else "ebc_lstm_grad", width, E, args.il_steps, h["il_stored"], h["il_episodes"], args.il_epochs, mark["il_s"]))
        mark["after_il"] = evaluate_saved(os.path.join(out_dir, "il_model.pth"), "after imitation learning")
        mark["t_rl"] = time.perf_counter()

    hist = run_lstm_training(env, trainer, space, gamma, il_steps=args.il_steps, il_epochs=args.il_epochs, train_iterations=args.iterations,
                             after_il=after_il, **common, **kw_om)
    torch.cuda.synchronize()
    rl_s = time.perf_counter() - mark["t_rl"]
    print("RL: %d rounds of %d decisions per env and %d optimizer steps of batch %d in %.2f s; loss first %.3e, last %.3e; replay memory %d"
          % (args.iterations, args.steps_per_iteration, args.train_batches, args.batch_size, rl_s,
             hist["rl_loss"][0] if hist["rl_loss"] else float("nan"), hist["rl_loss"][-1] if hist["rl_loss"] else float("nan"), hist["memory"]))
    env.close()
    trainer.save(args.out)
    print("saved %s" % args.out)
    after_rl = evaluate_saved(args.out, "after RL")
    print(json.dumps({"network": "ValueNetwork2" if two else "ValueNetwork1", "row_width": width, "envs": E, "il_steps": args.il_steps, "il_epochs": args.il_epochs, "il_stored": hist["il_stored"], "il_loss": hist["il_loss"],
                      "iterations": args.iterations, "rl_loss": [hist["rl_loss"][0], hist["rl_loss"][-1]] if hist["rl_loss"] else [],
                      "il_s": mark["il_s"], "rl_s": rl_s, "cases": args.cases, "after_il": mark["after_il"], "after_rl": after_rl}))


if __name__ == "__main__":
    main()
