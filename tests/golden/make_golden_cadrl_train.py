#!/usr/bin/env python3
"""Generate tests/golden/cadrl_one_trainer_steps.npz by importing the reference itself:

    python tests/golden/make_golden_cadrl_train.py --reference PATH_OF_THE_REFERENCE_TREE

Three optimizer steps of the reference's own Trainer (rl/utils/trainer.py:74-100, SGD momentum 0.9, learning rate 0.01)
on the reference's own CADRL ValueNetwork, built by its configure() after torch.manual_seed(11) like the networks of
make_golden_cadrl.py.  The states are the `last_state` vectors of the cadrl_one golden (the [13] joint states the
reference's transform gives with ONE other agent: R = 1), the targets their discounted returns over that run's rewards
(rl/utils/explorer.py:159-170 with gamma^(time_step * v_pref)).  The batches are fixed: step i trains on the states
BATCHES[i], the whole memory of that step as one batch, so the DataLoader's shuffle only permutes the mean.

Recorded: the states, the targets, the batch bounds, the loss of every step and every parameter before the first and
after each step.  Everything written is data."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_shims, jdump, parsed, save  # noqa: E402

SEED = 11
LEARNING_RATE = 0.01
BATCHES = [(0, 40), (40, 73), (73, 101)]


def gen(ref):
    import json
    import torch
    from rl.policy.policy_factory import policy_factory
    from rl.utils.memory import ReplayMemory
    from rl.utils.trainer import Trainer
    z = np.load(os.path.join(HERE, "cadrl_one.npz"), allow_pickle=True)
    meta = json.loads(str(z["meta"]))
    params = json.loads(str(z["params"]))
    states = z["last_state"].astype(np.float32)
    gamma_bar = float(meta["gamma"]) ** (float(params["time_step"]) * float(z["init_robot"][7]))
    values = np.zeros(len(states), dtype=np.float64)
    run = 0.0
    for t in range(len(states) - 1, -1, -1):
        run = float(z["reward"][t]) + gamma_bar * run
        values[t] = run
    values = values.astype(np.float32)
    torch.manual_seed(SEED)
    pol = policy_factory["cadrl"]()
    pol.configure(parsed(meta["policy_config_text"]))
    model = pol.get_model()
    out = {"states": states, "values": values, "batches": np.array(BATCHES), "lr": np.array(LEARNING_RATE),
           "gamma_bar": np.array(gamma_bar), "meta": jdump({"torch_seed": SEED, "source": "cadrl_one", "optimizer": "sgd"})}
    for k, v in model.state_dict().items():
        out["p0_" + k] = v.detach().numpy().copy()
    tr = Trainer(model, None, "cpu", 1, "sgd")
    tr.set_optimizer(LEARNING_RATE)
    losses = []
    for i, (a, b) in enumerate(BATCHES):
        mem = ReplayMemory(1000)
        for s, v in zip(states[a:b], values[a:b]):
            mem.push((torch.from_numpy(s), torch.Tensor([v])))
        tr.memory, tr.batch_size, tr.data_loader = mem, b - a, None
        losses.append(tr.optimize_batch(1))
        for k, v in model.state_dict().items():
            out["p%d_%s" % (i + 1, k)] = v.detach().numpy().copy()
    out["loss"] = np.array(losses)
    print("  losses", losses)
    save("cadrl_one_trainer_steps", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    args.reference = os.path.abspath(args.reference)
    install_shims()
    sys.path.insert(0, args.reference)
    os.chdir(args.reference)  # the reference resolves config paths relative to its root
    import logging
    logging.disable(logging.CRITICAL)
    gen(args.reference)


if __name__ == "__main__":
    main()
