"""Training the SAIL network by imitation on the device: demonstrations of the ORCA robot -> the fused forward + backward
kernel (ebc_sail_grad, csrc/ebc_sail_grad.h) -> a torch optimizer -> a state_dict in the reference's ExtendedNetwork
layout that tools/evaluate.py --policy sail loads.

SailTrainer keeps ONE flat float32 tensor in the kernel's packed layout (csrc/ebc_sail_rule.h: per layer W[k][64], then
bias[64], pad entries 0) as the master copy of the weights.  The kernel writes its .grad, any torch optimizer steps it,
ebc_sail_set_packed hands the result back to the network's handle.  native=False (and every CPU device) computes the same
loss and gradient with torch's autograd on SailModule: the comparison path, and what the CPU tests drive.

The loss is a plain regression on the demonstrator's action: mean squared error over the live envs' two outputs.  An env
is live (w_e = 1) unless it has arrived (SAIL's action is the constant (0, 0) there), its row count is not adult_num, or
its mask is 0; an env that is not live enters nothing.

After the behaviour cloning, DAgger (collect_dagger, DaggerDataset, dagger): the network drives the training envs, the ORCA
robot labels every state it visits in one ebc_sail_dagger_k call per round (csrc/ebc_dagger.h), and the fit runs on the
aggregate."""
import collections
import ctypes as C

import torch

from . import _abi
from .sail import HIDDEN, LAYERS, SailModule, SailNet, check_adult_num


def layer_shapes(adult_num):
    """[(in, out)] of the 14 Linear layers in the order of LAYERS (csrc/ebc_sail_rule.h: layer_in, layer_out)."""
    N = int(adult_num)
    return [(4, 32), (32, 32), (4 * N, 64), (64, 64), (64, 32), (64, 64), (64, 64), (64, 64), (64, 64), (64, 1), (4, 64),
            (64, 64), (128, 64), (64, 2)]


def packed_floats(adult_num):
    return sum((k + 1) * HIDDEN for k, _ in layer_shapes(adult_num))


def _layer_views(flat, adult_num):
    """Per layer (W view [out, in], bias view [out]) into a flat packed tensor."""
    out, at = [], 0
    for k, o in layer_shapes(adult_num):
        out.append((flat[at:at + k * HIDDEN].view(k, HIDDEN)[:, :o].t(), flat[at + k * HIDDEN:at + (k + 1) * HIDDEN][:o]))
        at += (k + 1) * HIDDEN
    return out


def pack_state_dict(sd, out=None):
    """A state_dict of the reference's keys -> the packed image, flat float32 [packed_floats] (on `out`'s device when a
    tensor to fill is given, else on the weights')."""
    N = int(sd["adult_encoder.0.weight"].shape[1]) // 4
    check_adult_num(N)
    if out is None:
        out = torch.zeros(packed_floats(N), dtype=torch.float32, device=sd["planner.weight"].device)
    else:
        out.zero_()
    with torch.no_grad():
        for key, (w, b) in zip(LAYERS, _layer_views(out, N)):
            w.copy_(sd[key + ".weight"])
            b.copy_(sd[key + ".bias"])
    return out


def unpack_to_state_dict(flat, adult_num):
    """The packed image -> an ordered state_dict with SailModule's (the reference's) keys, fresh contiguous tensors."""
    sd = collections.OrderedDict()
    for key, (w, b) in zip(LAYERS, _layer_views(flat.detach(), adult_num)):
        sd[key + ".weight"] = w.clone().contiguous()
        sd[key + ".bias"] = b.clone().contiguous()
    return sd  # LAYERS is SailModule's construction order, weight before bias: the reference's key order


def live_envs(robot, n_rows, mask, adult_num):
    """w_e as a bool tensor [E]: not arrived, adult_num rows, mask != 0."""
    w = ~(torch.sqrt((robot[:, 1] - robot[:, 6]) ** 2 + (robot[:, 0] - robot[:, 5]) ** 2) < robot[:, 4])
    if n_rows is not None:
        w = w & (n_rows.to(robot.device) == int(adult_num))
    if mask is not None:
        w = w & (mask.to(robot.device) != 0)
    return w


class SailTrainer(object):
    """module_or_state_dict: a SailModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "adam", "sgd" or a callable params -> torch optimizer.  native: the kernel (HIP devices only; the default there) or
    torch autograd."""

    def __init__(self, module_or_state_dict, device="cpu", optimizer="adam", lr=1e-3, native=None):
        sd = module_or_state_dict.state_dict() if isinstance(module_or_state_dict, torch.nn.Module) else module_or_state_dict
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items()}
        self.device = torch.device(device)
        self.adult_num = int(sd["adult_encoder.0.weight"].shape[1]) // 4
        check_adult_num(self.adult_num)
        self.native = (self.device.type == "cuda") if native is None else bool(native)
        if self.native and self.device.type != "cuda":
            raise NotImplementedError("SailTrainer(native=True) needs a HIP device: the kernel has no CPU form")
        self.flat = pack_state_dict(sd).to(self.device).requires_grad_(True)
        self.flat.grad = torch.zeros_like(self.flat)
        params = [self.flat]
        if callable(optimizer):
            self.optimizer = optimizer(params)
        elif optimizer == "adam":
            self.optimizer = torch.optim.Adam(params, lr=lr)
        elif optimizer == "sgd":
            self.optimizer = torch.optim.SGD(params, lr=lr, momentum=0.9)
        else:
            raise ValueError("optimizer: 'adam', 'sgd' or a callable")
        # the inference view on the same device: its native handle is the one the kernel trains (DeviceSailPolicy(trainer.net)
        # decides with the current weights); its torch module is the autograd path's
        self.net = SailNet(sd, device=self.device)
        self.module = self.net.module

    # ------------------------------------------------------------------ weights
    def state_dict(self):
        return unpack_to_state_dict(self.flat.detach().cpu(), self.adult_num)

    def save(self, path):
        """The current weights as a file torch.save wrote: loads into SailModule and the reference's ExtendedNetwork with
        strict=True."""
        torch.save(self.state_dict(), path)

    def _handle(self):
        return self.net.native()._h

    def push_weights(self):
        """The master copy into the network the policy objects use: ebc_sail_set_packed on the current stream (HIP), and
        the torch module's parameters."""
        if self.device.type == "cuda":
            from . import _capi
            _capi.check(_capi.lib().ebc_sail_set_packed(self._handle(), torch.cuda.current_stream(self.device).cuda_stream,
                                                        self.flat.data_ptr()))
        if not self.native:
            self._load_module()

    def _load_module(self):
        with torch.no_grad():
            views = _layer_views(self.flat.detach(), self.adult_num)
            mods = dict(self.module.named_parameters())
            for key, (w, b) in zip(LAYERS, views):
                mods[key + ".weight"].copy_(w)
                mods[key + ".bias"].copy_(b)

    # ------------------------------------------------------------------ loss and gradient
    def loss_and_grad(self, robot, ob, target, n_rows=None, mask=None, grad_scale=None, action=None):
        """robot [E, 9] float64, ob [E, R, 5] float64 (R >= adult_num), target [E, 2] float64, n_rows [E] int64 or None,
        mask [E] uint8 / bool or None, all on the trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64)
        there; .grad of the master copy holds d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 1 / count (the
        mean squared error; this reads the count back).  action [E, 2] float64, when given, receives the forward's
        actions (native only)."""
        N = self.adult_num
        robot, ob, target = robot.to(torch.float64).contiguous(), ob.to(torch.float64).contiguous(), target.to(torch.float64).contiguous()
        E, R = int(ob.shape[0]), int(ob.shape[1])
        if R < N:
            raise ValueError("SailTrainer: %d rows per env, the network takes exactly adult_num = %d" % (R, N))
        if grad_scale is None:
            grad_scale = 1.0 / max(int(live_envs(robot, n_rows, mask, N).sum()), 1)
        if self.native:
            return self._native_grad(robot, ob, target, n_rows, mask, float(grad_scale), action, E, R)
        if action is not None:
            raise NotImplementedError("SailTrainer(native=False): `action` is the kernel's output")
        w = live_envs(robot, n_rows, mask, N)
        self._load_module()
        params = [p for _, p in self.module.named_parameters()]
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        live = torch.nonzero(w).reshape(-1)
        if live.numel() == 0:
            self.flat.grad.zero_()
            return torch.zeros((), dtype=torch.float64, device=self.device), torch.zeros((), dtype=torch.int64, device=self.device)
        planned, _ = self.module(robot[live][:, [0, 1, 2, 3, 5, 6]].to(torch.float32).contiguous(),
                                 ob[live][:, :N, :4].to(torch.float32).contiguous())
        d = planned - target[live].to(torch.float32)
        (0.5 * float(grad_scale) * (d * d).sum()).backward()
        grads = {k: p.grad for k, p in self.module.named_parameters()}
        pack_state_dict(grads, out=self.flat.grad)
        for p in params:
            p.requires_grad_(False)
            p.grad = None
        return (d.detach().double() ** 2).sum(), torch.tensor(int(live.numel()), dtype=torch.int64, device=self.device)

    def _native_grad(self, robot, ob, target, n_rows, mask, grad_scale, action, E, R):
        from . import _capi
        dev = self.device
        loss, count = torch.empty((), dtype=torch.float64, device=dev), torch.empty((), dtype=torch.int64, device=dev)
        a = _abi.EbcSailGradArgs()
        a.struct_size = C.sizeof(a)
        a.E, a.R, a.grad_scale = E, R, grad_scale
        a.robot, a.ob, a.target = robot.data_ptr(), ob.data_ptr(), target.data_ptr()
        keep = []
        if n_rows is not None:
            keep.append(n_rows.to(device=dev, dtype=torch.int64).contiguous())
            a.n_rows = keep[-1].data_ptr()
        if mask is not None:
            keep.append(mask.to(device=dev).to(torch.uint8).contiguous())
            a.sample_mask = keep[-1].data_ptr()
        if action is not None:
            assert action.dtype == torch.float64 and action.is_contiguous() and tuple(action.shape) == (E, 2) and action.device == robot.device
            a.action = action.data_ptr()
        a.grad, a.loss_sum, a.count = self.flat.grad.data_ptr(), loss.data_ptr(), count.data_ptr()
        _capi.check(_capi.lib().ebc_sail_grad(self._handle(), torch.cuda.current_stream(dev).cuda_stream, C.addressof(a)))
        return loss, count

    def step(self):
        """Average the gradient over ranks (one all-reduce of the one tensor), step the optimizer, hand the weights on."""
        from .train import allreduce_flat_
        allreduce_flat_([self.flat])
        self.optimizer.step()
        self.push_weights()


def collect_sail_demos(env, steps, safety_space=0.15, persistent_sim=True, human_policy=_abi.HUMAN_ORCA, steps_per_call=None,
                       one_launch=False):
    """`steps` steps of every env of a BatchedEnv (on a HIP device, auto-reset) with the robot on ORCA, the demonstrator
    of rl/train.py:124-133 as train.collect_il runs it: per step the robot's FullState, the world-frame observation rows
    and the row counts go into [K, E, ...] buffers, ebc_robot_orca gives the action (the regression target, (vx, vy)),
    and the step takes it.  Kept: the steps of episodes that ended inside the window in ReachGoal.
    steps_per_call (an int K): the same window as ebc_step_k_world calls of at most K steps with EBC_ROBOT_ORCA, which
    write the same six buffers (world_robot, world_ob, n_rows, robot_action_out, done, info) without the host between
    the steps; one_launch: each call as one kernel launch (EBC_FLAG_ONE_LAUNCH; ORCA and by-type humans).  The dictionary is
    the loop's byte for byte.  None is the loop, five calls per step.
    -> dict(robot [M, 9], ob [M, R, 5], n_rows [M], target [M, 2], steps, episodes) on the device."""
    if int(env.params.robot_kinematics) != _abi.HOLONOMIC:
        raise NotImplementedError("collect_sail_demos: holonomic robots only: the demonstrator's action is (vx, vy), which SAIL "
                                  "emits as ActionXY; a unicycle robot's (v, r) targets are not built")
    dev = torch.device("cuda", env.device)
    K, E, R = int(steps), env.E, env.R
    env.robot_orca_sim(bool(persistent_sim))
    robot = torch.empty((K, E, 9), dtype=torch.float64, device=dev)
    ob = torch.empty((K, E, R, 5), dtype=torch.float64, device=dev)
    n_rows = torch.empty((K, E), dtype=torch.int64, device=dev)
    target = torch.empty((K, E, 2), dtype=torch.float64, device=dev)
    done = torch.empty((K, E), dtype=torch.uint8, device=dev)
    info = torch.empty((K, E), dtype=torch.uint8, device=dev)
    reward = torch.empty((E,), dtype=torch.float64, device=dev)
    if one_launch and steps_per_call is None:
        raise ValueError("collect_sail_demos: one_launch needs steps_per_call, the steps of a call")
    if steps_per_call is not None and int(steps_per_call) < 1:
        raise ValueError("collect_sail_demos: steps_per_call must be at least 1")
    flags = _abi.FLAG_AUTO_RESET | (_abi.FLAG_ONE_LAUNCH if one_launch else 0)
    for k0 in range(0, K if steps_per_call is not None else 0, int(steps_per_call or 1)):
        k1 = min(K, k0 + int(steps_per_call))
        env.step_k_device(dict(world_robot=robot[k0:k1], world_ob=ob[k0:k1], n_rows=n_rows[k0:k1], robot_action_out=target[k0:k1],
                               done=done[k0:k1], info=info[k0:k1]), k1 - k0, human_policy=human_policy,
                          robot_policy=_abi.ROBOT_ORCA, flags=flags, robot_safety_space=safety_space)
    for k in range(K if steps_per_call is None else 0):
        env.robot_state_device(robot[k])
        env.observe_ob_device(ob[k])
        env.row_counts_device(n_rows[k])
        env.robot_orca_device(target[k], safety_space)
        env.step_device(dict(reward=reward, done=done[k], info=info[k]), robot_action=target[k], human_policy=human_policy,
                        flags=_abi.FLAG_AUTO_RESET)
    env.synchronize()
    keep = torch.zeros((K, E), dtype=torch.bool, device=dev)
    closed = torch.zeros((E,), dtype=torch.bool, device=dev)
    for k in range(K - 1, -1, -1):  # backwards: a step is kept when the next terminal step of its env is a ReachGoal
        closed = torch.where(done[k].bool(), info[k] == _abi.INFO_REACH_GOAL, closed)
        keep[k] = closed
    keep = keep.reshape(-1)
    return dict(robot=robot.reshape(K * E, 9)[keep], ob=ob.reshape(K * E, R, 5)[keep], n_rows=n_rows.reshape(-1)[keep],
                target=target.reshape(K * E, 2)[keep], steps=int(keep.sum()), episodes=int(done.sum()))


def fit(trainer, demos, epochs, batch_size, generator=None):
    """`epochs` shuffled passes over the kept samples in minibatches: loss_and_grad plus a step each -> the per-epoch mean
    losses (mean squared error per output element, weighted by the batches' live envs)."""
    n = int(demos["robot"].shape[0])
    if n == 0:
        raise ValueError("no demonstrations were kept: no episode ended in ReachGoal inside the window")
    dev = demos["robot"].device
    losses = []
    for _ in range(int(epochs)):
        perm = torch.randperm(n, device=dev, generator=generator)
        total = torch.zeros((), dtype=torch.float64, device=dev)
        counted = torch.zeros((), dtype=torch.int64, device=dev)
        for b in range(0, n, int(batch_size)):
            idx = perm[b:b + int(batch_size)]
            # the kept steps are live but for a row count other than adult_num; a batch's scale is its size
            loss, count = trainer.loss_and_grad(demos["robot"][idx], demos["ob"][idx], demos["target"][idx], demos["n_rows"][idx],
                                                grad_scale=1.0 / int(idx.numel()))
            trainer.step()
            total += loss
            counted += count
        losses.append(float(total) / max(2 * int(counted), 1))
    return losses


def train_sail(env, trainer, demo_steps, epochs, batch_size, generator=None, safety_space=0.15, persistent_sim=True,
               steps_per_call=None, one_launch=False):
    """Demonstrations from `env`, then the fit -> the per-epoch mean losses."""
    demos = collect_sail_demos(env, demo_steps, safety_space, persistent_sim, steps_per_call=steps_per_call, one_launch=one_launch)
    return fit(trainer, demos, epochs, batch_size, generator)


# ---------------------------------------------------------------------- DAgger (Ross, Gordon and Bagnell 2011)
# Behaviour cloning sees the demonstrator's own states only.  A DAgger round lets the LEARNER drive (mixed with the expert
# with probability beta), has the expert label every state the learner visits, adds those to the aggregate and fits again.

def dagger_beta(round_index, beta0=0.5, beta_decay=0.5):
    """The probability that a step of round i >= 1 executes the expert's action: beta0 * beta_decay ** (i - 1)."""
    if round_index < 1:
        raise ValueError("round 0 is behaviour cloning: the expert drives every step")
    return float(beta0) * float(beta_decay) ** (int(round_index) - 1)


def dagger_mask(steps, n_envs, beta, device, generator=None):
    """take_expert [K, E] bool on `device`: torch.rand < beta from the generator (reproducible from its seed); None at
    beta <= 0 (the learner always acts, the entry's NULL)."""
    if not beta > 0.0:
        return None
    return torch.rand((int(steps), int(n_envs)), device=device, generator=generator) < float(beta)


def collect_dagger(env, steps, beta, generator=None, safety_space=0.15, human_policy=_abi.HUMAN_ORCA):
    """One DAgger window: `steps` closed-loop steps of every env of a BatchedEnv (HIP device, auto-reset) in ONE
    ebc_sail_dagger_k call — the network attached to `env` drives, a step executes the expert's action instead with
    probability beta, and the ORCA robot labels every visited state.  Kept: the samples whose env is live (live_envs:
    not arrived, adult_num rows) and whose expert action is finite; there is no ReachGoal filter, the states where the
    learner went wrong are the point.
    -> the dict of collect_sail_demos (robot [M, 9], ob [M, R, 5], n_rows [M], target [M, 2] = the expert's action,
    steps, episodes) plus executed [M, 2], learner [M, 2], `window` = the [K, E, ...] outputs and `take_expert` as the
    call had them, `keep` [K * E] bool, and the window's outcome counts success / collision / timeout."""
    if int(env.params.robot_kinematics) != _abi.HOLONOMIC:
        raise NotImplementedError("collect_dagger: holonomic robots only: the expert's action is (vx, vy)")
    net = getattr(env, "_sail", None)
    if net is None:
        raise ValueError("collect_dagger: no SAIL network attached to the env (BatchedEnv.attach_sail)")
    dev = torch.device("cuda", env.device)
    K, E, R = int(steps), env.E, env.R
    out = env.alloc_sail_dagger_outputs(K)
    take = dagger_mask(K, E, beta, dev, generator)
    # the mask and the trainer's last weights are work of torch's stream; the handle's stream may be another
    torch.cuda.current_stream(dev).synchronize()
    env.sail_dagger_k_device(out, K, take_expert=take, safety_space=safety_space, human_policy=human_policy,
                             flags=_abi.FLAG_AUTO_RESET)
    env.synchronize()
    robot, n_rows, expert = out["robot"].reshape(K * E, 9), out["n_rows"].reshape(-1), out["expert_action"].reshape(K * E, 2)
    keep = live_envs(robot, n_rows, None, net.adult_num) & torch.isfinite(expert).all(dim=1)
    done, info = out["done"].bool(), out["info"]
    collision = (info >= _abi.INFO_COLLISION_OBSTACLE) & (info <= _abi.INFO_COLLISION_CHILD)
    return dict(robot=robot[keep], ob=out["ob"].reshape(K * E, R, 5)[keep], n_rows=n_rows[keep], target=expert[keep],
                executed=out["robot_action_out"].reshape(K * E, 2)[keep], learner=out["learner_action"].reshape(K * E, 2)[keep],
                steps=int(keep.sum()), episodes=int(done.sum()), success=int((done & (info == _abi.INFO_REACH_GOAL)).sum()),
                collision=int((done & collision).sum()), timeout=int((done & (info == _abi.INFO_TIMEOUT)).sum()),
                keep=keep, window=out, take_expert=take)


_SAMPLE_KEYS = ("robot", "ob", "n_rows", "target")


class DaggerDataset(object):
    """The aggregate of DAgger: samples appended in order, on whatever device they arrive on; past `capacity` samples the
    oldest leave first (FIFO)."""

    def __init__(self, capacity):
        if int(capacity) < 1:
            raise ValueError("capacity >= 1")
        self.capacity = int(capacity)
        self.data = None

    def __len__(self):
        return 0 if self.data is None else int(self.data["robot"].shape[0])

    def append(self, samples):
        new = {k: samples[k] for k in _SAMPLE_KEYS}
        if self.data is not None:
            new = {k: torch.cat([self.data[k], new[k]], dim=0) for k in _SAMPLE_KEYS}
        n = int(new["robot"].shape[0])
        if n > self.capacity:
            new = {k: v[n - self.capacity:].clone() for k, v in new.items()}  # a copy: the dropped samples' memory goes
        self.data = new
        return len(self)

    def as_demos(self):
        """The dict fit() takes."""
        if self.data is None:
            raise ValueError("the dataset is empty")
        return dict(self.data, steps=len(self))


def dagger(env, trainer, rounds, demo_steps, dagger_steps, epochs, dagger_epochs, batch_size, beta0=0.5, beta_decay=0.5,
           capacity=1 << 20, generator=None, safety_space=0.15, on_round=None, persistent_sim=True, demo_steps_per_call=None,
           demo_one_launch=False):
    """Round 0: collect_sail_demos + fit, exactly train_sail.  Round i >= 1: collect_dagger at beta0 * beta_decay^(i - 1)
    on `env` (the env trainer.net is attached to: SailTrainer.step has already handed it the new weights), append to the
    aggregate, fit on all of it for dagger_epochs.  on_round(i, info) runs after every round's fit; info holds round,
    beta, losses, samples (this round's), aggregate, episodes and, from round 1 on, the window's outcome counts.
    -> (per-round list of the per-epoch losses, the DaggerDataset).  rounds = 0 is train_sail."""
    data = DaggerDataset(capacity)
    demos = collect_sail_demos(env, demo_steps, safety_space, persistent_sim, steps_per_call=demo_steps_per_call,
                               one_launch=demo_one_launch)  # round 0 in windows of ebc_step_k_world, when asked for
    if int(rounds) > 0:
        data.append(demos)
    losses = [fit(trainer, demos, epochs, batch_size, generator)]
    if on_round is not None:
        on_round(0, dict(round=0, beta=1.0, losses=losses[0], samples=demos["steps"], aggregate=demos["steps"],
                         episodes=demos["episodes"]))
    for i in range(1, int(rounds) + 1):
        env.attach_sail(trainer.net)
        beta = dagger_beta(i, beta0, beta_decay)
        got = collect_dagger(env, dagger_steps, beta, generator, safety_space)
        data.append(got)
        losses.append(fit(trainer, data.as_demos(), dagger_epochs, batch_size, generator))
        if on_round is not None:
            on_round(i, dict(round=i, beta=beta, losses=losses[-1], samples=got["steps"], aggregate=len(data),
                             episodes=got["episodes"], success=got["success"], collision=got["collision"],
                             timeout=got["timeout"]))
    return losses, data
