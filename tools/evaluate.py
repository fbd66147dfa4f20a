#!/usr/bin/env python3
"""What rl/test.py does with a trained model (rl/test.py:99-151 -> Explorer.run_k_episodes over the test
cases, rl/utils/explorer.py:116-131), on the device: `--cases` test cases (seed 1000 + case, the reference's
"test" phase) as one batch, the SARL value network from a reference .pth driving every robot, the
reference's metrics at the end.

    python3 tools/evaluate.py --weights tests/golden/weights/sarl_n10_ebcadrl.pth \
        --env-config eb-cadrl_amd/configs/bench_metric.config --policy-config eb-cadrl_amd/configs/policy_agent_type.config \
        --cases 1000 [--policy orca]     (orca: the imitation-learning demonstrator instead of the network)
    python3 tools/evaluate.py --policy-config OM_POLICY_CONFIG --weights OM_SARL_STATE_DICT_FILE
                                         (sarl with [sarl] with_om = true in the policy config: OM-SARL, the occupancy maps
                                          of its [om] section appended to every row on the device; no tree ships OM
                                          weights: --weights is required, what rl/train.py saved)
    python3 tools/evaluate.py --policy lstm_rl --weights LSTM_RL_STATE_DICT_FILE
                                         (lstm_rl: the LSTM-RL value network, either of the reference's two; rows 13
                                          wide whatever [sarl] says.  The reference ships no trained LSTM-RL model and
                                          the repository carries none: --weights is required, what rl/train.py saved)
    python3 tools/evaluate.py --policy lstm_rl --policy-config eb-cadrl_amd/configs/policy_om_lstm.config --weights OM_LSTM_FILE
                                         (lstm_rl with [lstm_rl] with_om = true in the policy config: OM-LSTM, the
                                          occupancy maps of its [om] section appended to every row on the device, rows
                                          13 + 48 = 61 wide; --weights is required, what tools/train_lstm.py saved)
    python3 tools/evaluate.py --policy cadrl --weights CADRL_STATE_DICT_FILE
                                         (cadrl: the CADRL value network, value_network.{0,2,4,6}; the minimum over the
                                          rows and the choice are one kernel.  Rows 13 wide; neither tree ships a
                                          trained CADRL model: --weights is required)
    python3 tools/evaluate.py --policy sail --weights SAIL_STATE_DICT_FILE --env-config ENV_WITH_ADULT_NUM_ROWS
                                         (sail: the SAIL network, one kernel from the device state to the action, no
                                          look-ahead; every scene must have exactly the network's adult_num rows, an
                                          env with another count gets a NaN action.  Neither tree ships SAIL weights:
                                          --weights is required)
    python3 tools/evaluate.py --policy sail --weights SAIL_STATE_DICT_FILE --env-config ENV --steps-per-call 32 [--one-launch]
                                         (the same episodes in windows of 32 steps per ebc_step_k call with the network
                                          as the robot policy on the device, EBC_ROBOT_SAIL: same metrics, no host
                                          work per step; --one-launch: each window as one kernel launch)
    python3 tools/evaluate.py ... --record episodes.npz
                                         (any policy, either loop: the robot's state and the world-frame rows before every
                                          step of every case, cut at its terminal step, with length, final, the humans'
                                          types and the case indices: what a trajectory plot of a listed case needs)
"""
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default=None, help="a reference state_dict file (default for sarl: tests/golden/weights/sarl_n10_ebcadrl.pth; "
                    "required for --policy lstm_rl, --policy cadrl and --policy sail)")
    ap.add_argument("--env-config", default=os.path.join(ROOT, "eb-cadrl_amd", "configs", "bench_metric.config"))
    ap.add_argument("--policy-config", default=os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    ap.add_argument("--cases", type=int, default=1000)
    ap.add_argument("--first-case", type=int, default=0)
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--policy", default="sarl", choices=["sarl", "lstm_rl", "cadrl", "sail", "orca"])
    ap.add_argument("--safety-space", type=float, default=0.15)
    ap.add_argument("--device-scenes", action="store_true",
                    help="generate the test scenes on the device (ebc_generate_reset) instead of on the host")
    ap.add_argument("--steps-per-call", type=int, default=0, metavar="K",
                    help="--policy sail: advance in windows of K steps per ebc_step_k call (default 0: the per-step loop)")
    ap.add_argument("--one-launch", action="store_true", help="with --steps-per-call: each window as one kernel launch")
    ap.add_argument("--record", default=None, metavar="PATH",
                    help="save every case's world-frame trajectory (ebcsim.record.EpisodeRecorder) as one .npz")
    ap.add_argument("--wide-decide", action="store_true",
                    help="--policy sarl: stacks wider than the two-layer block (up to 640 units: policy_x3 / policy_x4) as wide blocks instead of torch")
    args = ap.parse_args()
    if (args.steps_per_call or args.one_launch) and args.policy != "sail":
        ap.error("--steps-per-call / --one-launch go with --policy sail, the policy ebc_step_k keeps on the device")
    if args.one_launch and args.steps_per_call < 1:
        ap.error("--one-launch needs --steps-per-call K")
    if args.policy == "lstm_rl" and not args.weights:
        ap.error("--policy lstm_rl needs --weights: a state_dict file of one of the reference's LSTM-RL networks")
    if args.policy == "cadrl" and not args.weights:
        ap.error("--policy cadrl needs --weights: a state_dict file of the reference's CADRL network")
    if args.policy == "sail" and not args.weights:
        ap.error("--policy sail needs --weights: a state_dict file of the reference's SAIL network (ExtendedNetwork)")
    pol_cfg = configparser.RawConfigParser()
    pol_cfg.read(args.policy_config)
    with_om = args.policy == "sarl" and pol_cfg.getboolean("sarl", "with_om", fallback=False)
    lstm_om = args.policy == "lstm_rl" and pol_cfg.getboolean("lstm_rl", "with_om", fallback=False)
    if with_om and not args.weights:
        ap.error("--policy sarl with [sarl] with_om = true needs --weights: a state_dict file of an OM-SARL network (no tree ships one)")
    import torch
    from ebcsim import _abi, actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    from ebcsim.train import evaluate
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(args.env_config)
    pol.read(args.policy_config)
    params = ebc_config.params_from_config(cfg, pol, policy=args.policy)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    weights = args.weights or os.path.join(ROOT, "tests", "golden", "weights", "sarl_n10_ebcadrl.pth")
    t0 = time.perf_counter()
    seeds = [ebc_scene.COUNTER_OFFSET["test"] + args.first_case + c for c in range(args.cases)]
    if args.device_scenes:
        gen = ebc_scene.gen_struct(sc, "test")
        env = BatchedEnv(params, args.cases, sum(gen.count), ebc_scene.max_static_rows(sc))
        env.generate_reset(gen, seeds[0])
        env.synchronize()
        v_pref = sc.robot.v_pref
    else:
        batch = ebc_scene.SceneBatch.from_scenes([ebc_scene.generate_scene(sc, s, "test") for s in seeds])
        env = BatchedEnv(params, args.cases, batch.N, batch.S)
        env.reset(batch)
        v_pref = float(batch.robot[0, 7])
    t1 = time.perf_counter()
    env.use_torch_stream()
    # the humans' policy is the env config's ([adults] / [bicycles] / [children] policy; a mix runs EBC_HUMAN_BY_TYPE):
    # what asks for HUMAN_ORCA below runs it
    env.configure_humans(*ebc_config.human_policies_from_config(cfg))
    if args.policy in ("sarl", "lstm_rl", "cadrl"):
        make_policy = DeviceSarlPolicy
        if args.policy == "lstm_rl":
            from ebcsim.lstm_rl import LstmValueNet
            net = LstmValueNet.load(weights, device="cuda:0")
        elif args.policy == "cadrl":
            from ebcsim.cadrl import CadrlValueNet, DeviceCadrlPolicy
            net, make_policy = CadrlValueNet.load(weights, device="cuda:0"), DeviceCadrlPolicy
        else:
            net = SarlValueNet.load(weights, device="cuda:0", **({"wide": True} if args.wide_decide else {}))
        kw = {}
        if with_om:
            kw["om"] = ebc_config.occupancy_from_config(pol, policy=args.policy)
        if lstm_om:
            kw["om"] = ebc_config.occupancy_from_config(pol, policy="om_lstm_rl")
        policy = make_policy(net, ebc_actions.build_action_space(v_pref), args.gamma, **kw)
        decide, hp = (lambda e: policy.decide(e)[0]), _abi.HUMAN_CACHED
    elif args.policy == "sail":
        from ebcsim.sail import DeviceSailPolicy, SailNet
        policy = DeviceSailPolicy(SailNet.load(weights, device="cuda:0"))
        # no look-ahead, so no human velocities are cached: the humans' own policy runs inside the step
        decide, hp = (lambda e: policy.decide(e)[0]), _abi.HUMAN_ORCA
    else:
        act = torch.zeros((args.cases, 2), dtype=torch.float64, device="cuda:0")

        def decide(e):
            e.robot_orca_device(act, args.safety_space)
            return act
        hp = _abi.HUMAN_ORCA
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rec = None
    if args.record:
        from ebcsim.record import EpisodeRecorder
        rec = EpisodeRecorder(env, int(round(params.time_limit / params.time_step)) + 2)  # the steps evaluate() takes at most
        rec.case += args.first_case
    if args.steps_per_call > 0:
        from ebcsim.train import evaluate_windows
        flags = _abi.FLAG_ONE_LAUNCH if args.one_launch else 0
        rollout = lambda e, K, outs: policy.rollout(e, K, outs, flags=flags, human_policy=hp)  # noqa: E731
        m = evaluate_windows(env, rec.recording(rollout) if rec is not None else rollout, args.gamma, args.steps_per_call)
    else:
        m = evaluate(env, decide, args.gamma, human_policy=hp, record=rec)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    if rec is not None:
        print("recorded %d cases to %s" % (args.cases, rec.save(args.record)))
    print("TEST  has success rate: %.2f, collision rate adult / bicycle / child / obstacle: %.2f / %.2f / %.2f / %.4f, "
          "timeout: %d, nav time: %.2f, total reward: %.4f" % (
              m["success_rate"], m["collision_rate_adult"], m["collision_rate_bicycle"], m["collision_rate_child"],
              m["collision_rate_obstacle"], m["timeout"], m["avg_nav_time"], m["total_reward:"]))
    print("Frequency of being in danger: %.2f and average min separate distance in danger: %.2f" % (
        m["Frequency of being in danger"] or 0.0, m["average min separate distance in danger"]))
    print(json.dumps({"cases": args.cases, "policy": args.policy, "scenes": "device" if args.device_scenes else "host", "scene_generation_s": t1 - t0, "episodes_s": t3 - t2,
                      "episodes_per_s": args.cases / (t3 - t2),
                      "metrics": {k: v for k, v in m.items() if not isinstance(v, list)}}))


if __name__ == "__main__":
    main()
