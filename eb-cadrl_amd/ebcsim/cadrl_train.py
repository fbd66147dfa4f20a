"""Training the CADRL value network on the device: rollouts -> the fused forward + minimum + backward kernel
(ebc_cadrl_grad, csrc/ebc_cadrl_grad.h) -> a torch optimizer -> a state_dict in the reference's ValueNetwork layout
(value_network.{0,2,4,6}.{weight,bias}) that tools/evaluate.py --policy cadrl loads.

CadrlTrainer keeps ONE flat float32 tensor in the kernel's packed layout (csrc/ebc_cadrl_grad_rule.h: per layer W[k][units
padded to a multiple of 4], then the bias, pad entries 0) as the master copy of the weights.  The kernel writes its .grad,
a torch optimizer steps it, ebc_cadrl_net_set_packed hands the result back to the kernel's network object and
CadrlValueNet.refresh_native hands it to the two-layer blocks that decide.  native=False (and every CPU device) computes
the same loss and gradient with torch's autograd on CadrlModule: the comparison path, and what the CPU tests drive.

The loss is the reference's (rl/utils/trainer.py:74-100): the mean squared error between the network's value of a state
and its target.  The reference trains CADRL on one-human scenes only, because its transform asserts a single other agent
(rl/policy/cadrl.py:224-234): a state is one row and the value is the network's output on it.  A state with R > 1 rows is
worth the MINIMUM over its rows here, as the decision takes it, and the gradient flows through the first row that holds the
minimum: that is this project's batched extension, not something the reference trains.  With R = 1 the two are the same.

run_cadrl_training is the schedule of rl/train.py:99-260 on the generic pieces of ebcsim.train (collect_il, collect,
EpisodeStore, DeviceReplay) with this trainer in the optimizer's place."""
import collections
import ctypes as C
import os

import torch

from . import _abi
from .cadrl import CadrlModule, CadrlValueNet, DeviceCadrlPolicy

LAYER_KEYS = ("value_network.0", "value_network.2", "value_network.4", "value_network.6")
MAX_IN, MAX_WIDTH, MAX_ROWS = 64, 256, 128  # csrc/ebc_cadrl_grad_rule.h, csrc/ebc_cadrl_rule.h


def pad4(n):
    return (int(n) + 3) & ~3


def widths_of(sd):
    """[row width, units of layer 1 .. 4] of a state_dict with the reference's keys."""
    keys = sorted(k for k in sd if k.startswith("value_network.") and k.endswith(".weight"))
    if [k[:-len(".weight")] for k in keys] != list(LAYER_KEYS):
        raise NotImplementedError("CADRL training: value_network is four Linear layers (value_network.0, .2, .4, .6), got %s" % keys)
    return [int(sd[LAYER_KEYS[0] + ".weight"].shape[1])] + [int(sd[k + ".weight"].shape[0]) for k in LAYER_KEYS]


def packed_floats(widths):
    return sum((k + 1) * pad4(o) for k, o in zip(widths[:-1], widths[1:]))


def _layer_views(flat, widths):
    """Per layer (W view [out, in], bias view [out]) into a flat packed tensor."""
    out, at = [], 0
    for k, o in zip(widths[:-1], widths[1:]):
        op = pad4(o)
        out.append((flat[at:at + k * op].view(k, op)[:, :o].t(), flat[at + k * op:at + (k + 1) * op][:o]))
        at += (k + 1) * op
    return out


def pack_state_dict(sd, out=None):
    """A state_dict of the reference's keys -> the packed image, flat float32 (into `out` when given)."""
    widths = widths_of(sd)
    if out is None:
        out = torch.zeros(packed_floats(widths), dtype=torch.float32, device=sd[LAYER_KEYS[0] + ".weight"].device)
    else:
        out.zero_()
    with torch.no_grad():
        for key, (w, b) in zip(LAYER_KEYS, _layer_views(out, widths)):
            w.copy_(sd[key + ".weight"])
            b.copy_(sd[key + ".bias"])
    return out


def unpack_to_state_dict(flat, widths):
    """The packed image -> an ordered state_dict with CadrlModule's (the reference's) keys, fresh contiguous tensors."""
    sd = collections.OrderedDict()
    for key, (w, b) in zip(LAYER_KEYS, _layer_views(flat.detach(), widths)):
        sd[key + ".weight"] = w.clone().contiguous()
        sd[key + ".bias"] = b.clone().contiguous()
    return sd


def live_states(B, R, n_valid, mask, device):
    """live as a bool tensor [B]: mask != 0 and at least one row."""
    w = torch.ones(B, dtype=torch.bool, device=device)
    if n_valid is not None:
        w = w & (n_valid.to(device) >= 1)
    if mask is not None:
        w = w & (mask.to(device) != 0)
    return w


class CadrlNet(object):
    """The kernel's network object (ebc_cadrl_net_*): the packed image of a state_dict in device memory."""

    def __init__(self, sd, device_index):
        from . import _capi
        self._L = _capi.lib()
        self.widths = widths_of(sd)
        host = [(sd[k + ".weight"].detach().to("cpu", torch.float32).contiguous().numpy(),
                 sd[k + ".bias"].detach().to("cpu", torch.float32).contiguous().numpy()) for k in LAYER_KEYS]
        w = _abi.EbcCadrlNetWeights()
        w.struct_size = C.sizeof(w)
        w.n_layers = len(LAYER_KEYS)
        for i, v in enumerate(self.widths):
            w.widths[i] = v
        for i, (a, b) in enumerate(host):
            w.weight[i], w.bias[i] = a.ctypes.data, b.ctypes.data
        self._h = C.c_void_p()
        _capi.check(self._L.ebc_cadrl_net_create(C.addressof(w), int(device_index), C.byref(self._h)))

    def packed_floats(self):
        from . import _capi
        n = C.c_int64()
        _capi.check(self._L.ebc_cadrl_net_packed_floats(self._h, C.byref(n)))
        return int(n.value)

    def get_packed(self, out):
        from . import _capi
        assert out.dtype == torch.float32 and out.is_contiguous() and out.is_cuda and out.numel() == self.packed_floats()
        _capi.check(self._L.ebc_cadrl_net_get_packed(self._h, torch.cuda.current_stream(out.device).cuda_stream, out.data_ptr()))
        return out

    def set_packed(self, flat):
        from . import _capi
        assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.is_cuda and flat.numel() == self.packed_floats()
        _capi.check(self._L.ebc_cadrl_net_set_packed(self._h, torch.cuda.current_stream(flat.device).cuda_stream, flat.data_ptr()))

    def grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, min_row=None):
        """One ebc_cadrl_grad on the current stream: rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None,
        mask [B] uint8 or None -> grad [packed floats], loss_sum 0-d float64, count 0-d int64, value [B] float32 and
        min_row [B] int32 when given; every tensor contiguous on the network's device."""
        from . import _capi
        B, R, T = (int(x) for x in rows.shape)
        a = _abi.EbcCadrlGradArgs()
        a.struct_size = C.sizeof(a)
        a.B, a.R, a.T, a.grad_scale = B, R, T, float(grad_scale)
        for name, t, dtype, numel in (("rows", rows, torch.float32, B * R * T), ("target", target, torch.float32, B),
                                      ("n_valid", n_valid, torch.int64, B), ("sample_mask", mask, torch.uint8, B),
                                      ("grad", grad, torch.float32, self.packed_floats()), ("loss_sum", loss_sum, torch.float64, 1),
                                      ("count", count, torch.int64, 1), ("value", value, torch.float32, B),
                                      ("min_row", min_row, torch.int32, B)):
            if t is None:
                continue
            assert t.dtype == dtype and t.is_contiguous() and t.is_cuda and t.numel() == numel, name
            setattr(a, name, t.data_ptr())
        _capi.check(self._L.ebc_cadrl_grad(self._h, torch.cuda.current_stream(rows.device).cuda_stream, C.addressof(a)))

    def __del__(self):
        try:
            self._L.ebc_cadrl_net_destroy(self._h)
        except Exception:
            pass


class CadrlTrainer(object):
    """module_or_state_dict: a CadrlModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "sgd" (momentum 0.9), "adam" (rl/utils/trainer.py:24-45) or a callable params -> torch optimizer.  native: the kernel
    (HIP devices only; the default there) or torch autograd of CadrlModule."""

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None):
        sd = module_or_state_dict.state_dict() if isinstance(module_or_state_dict, torch.nn.Module) else module_or_state_dict
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items()}
        self.device = torch.device(device)
        self.widths = widths_of(sd)
        self.native = (self.device.type == "cuda") if native is None else bool(native)
        if self.native and self.device.type != "cuda":
            raise NotImplementedError("CadrlTrainer(native=True) needs a HIP device: the kernel has no CPU form")
        self.flat = pack_state_dict(sd).to(self.device).requires_grad_(True)
        self.flat.grad = torch.zeros_like(self.flat)
        self._optimizer_spec = optimizer
        self.set_learning_rate(lr)
        self.module = CadrlModule.from_state_dict(sd).to(self.device)  # the autograd path's
        self.net = None
        if self.native:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.net = CadrlNet(sd, idx)

    def set_learning_rate(self, lr):
        """Trainer.set_optimizer (trainer.py:24-45): a new optimizer at the stage's learning rate."""
        spec, params = self._optimizer_spec, [self.flat]
        if callable(spec):
            self.optimizer = spec(params)
        elif spec == "adam":
            self.optimizer = torch.optim.Adam(params, lr=lr)
        elif spec == "sgd":
            self.optimizer = torch.optim.SGD(params, lr=lr, momentum=0.9)
        else:
            raise ValueError("optimizer: 'sgd', 'adam' or a callable")

    # ------------------------------------------------------------------ weights
    def state_dict(self):
        return unpack_to_state_dict(self.flat.detach().cpu(), self.widths)

    def device_state_dict(self):
        """The reference's keys as views into the master copy on its device (no copy): what refresh_native re-packs from."""
        sd = collections.OrderedDict()
        for key, (w, b) in zip(LAYER_KEYS, _layer_views(self.flat.detach(), self.widths)):
            sd[key + ".weight"], sd[key + ".bias"] = w, b
        return sd

    def save(self, path):
        """The current weights as a file torch.save wrote: loads into CadrlModule and the reference's ValueNetwork with
        strict=True."""
        torch.save(self.state_dict(), path)

    def load_state_dict(self, sd):
        if widths_of(sd) != self.widths:
            raise ValueError("CadrlTrainer.load_state_dict: other layer widths")
        with torch.no_grad():
            pack_state_dict({k: v.to(self.device, torch.float32) for k, v in sd.items()}, out=self.flat)
        self.push_weights()

    def push_weights(self):
        """The master copy into the kernel's network object (ebc_cadrl_net_set_packed on the current stream)."""
        if self.net is not None:
            self.net.set_packed(self.flat.detach())

    def _load_module(self):
        with torch.no_grad():
            params = dict(self.module.named_parameters())
            for key, (w, b) in zip(LAYER_KEYS, _layer_views(self.flat.detach(), self.widths)):
                params[key + ".weight"].copy_(w)
                params[key + ".bias"].copy_(b)

    # ------------------------------------------------------------------ loss and gradient
    def loss_and_grad(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, min_row=None):
        """rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None, mask [B] uint8 / bool or None, on the
        trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64) there; .grad of the master copy holds
        d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 2 / count, torch's MSELoss over the live states (this
        reads the count back).  value [B] float32 / min_row [B] int32, when given, receive the states' values and the
        rows they came from (native only)."""
        rows, target = rows.to(self.device, torch.float32).contiguous(), target.to(self.device, torch.float32).reshape(-1).contiguous()
        B, R, T = (int(x) for x in rows.shape)
        if T != self.widths[0]:
            raise ValueError("CadrlTrainer: rows are %d wide, the network takes %d" % (T, self.widths[0]))
        live = None
        if grad_scale is None:
            live = live_states(B, R, n_valid, mask, self.device)
            grad_scale = 2.0 / max(int(live.sum()), 1)
        if self.native:
            loss = torch.empty((), dtype=torch.float64, device=self.device)
            count = torch.empty((), dtype=torch.int64, device=self.device)
            nv = None if n_valid is None else n_valid.to(device=self.device, dtype=torch.int64).contiguous()
            mk = None if mask is None else mask.to(device=self.device).to(torch.uint8).contiguous()
            self.net.grad(rows, target, self.flat.grad, loss, count, grad_scale, nv, mk, value, min_row)
            return loss, count
        if value is not None or min_row is not None:
            raise NotImplementedError("CadrlTrainer(native=False): `value` and `min_row` are the kernel's outputs")
        if live is None:
            live = live_states(B, R, n_valid, mask, self.device)
        idx = torch.nonzero(live).reshape(-1)
        if idx.numel() == 0:
            self.flat.grad.zero_()
            return torch.zeros((), dtype=torch.float64, device=self.device), torch.zeros((), dtype=torch.int64, device=self.device)
        self._load_module()
        params = list(self.module.parameters())
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        x, nv = rows[idx], None
        if n_valid is not None:
            # rows past a state's own are never read by the kernel; autograd multiplies their (zero) deltas with them, so
            # a NaN there must not be an input
            nv = n_valid.to(self.device)[idx].clamp(max=R)
            x = torch.where((torch.arange(R, device=self.device)[None, :] < nv[:, None])[:, :, None], x, torch.zeros_like(x))
        out = self.module(x, nv)
        d = out - target[idx]
        (0.5 * float(grad_scale) * (d * d).sum()).backward()
        pack_state_dict({k: p.grad for k, p in self.module.named_parameters()}, out=self.flat.grad)
        for p in params:
            p.requires_grad_(False)
            p.grad = None
        return (d.detach().double() ** 2).sum(), torch.tensor(int(idx.numel()), dtype=torch.int64, device=self.device)

    def step(self):
        """Average the gradient over ranks (one all-reduce of the one tensor), step the optimizer, hand the weights on."""
        from .train import allreduce_flat_
        allreduce_flat_([self.flat])
        self.optimizer.step()
        self.push_weights()


def optimize_epoch(trainer, memory, num_epochs, batch_size, generator=None):
    """Trainer.optimize_epoch (trainer.py:45-72, imitation learning) with CadrlTrainer: `num_epochs` shuffled passes over
    the memory in batches; all ranks take the same number of batches (the smallest shard's).  -> the last epoch's summed
    batch losses divided by len(memory), as the reference reports it."""
    import torch.distributed as dist
    n, bs = len(memory), int(batch_size)
    batches = (n + bs - 1) // bs
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([batches], dtype=torch.int64, device=memory.states.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        batches = int(t.item())
    average = 0.0
    for _ in range(int(num_epochs)):
        perm = torch.randperm(n, device=memory.states.device, generator=generator)
        total = torch.zeros((), dtype=torch.float64, device=memory.states.device)
        for b in range(batches):
            idx = perm[b * bs:(b + 1) * bs]
            loss, _ = trainer.loss_and_grad(memory.states[idx], memory.values[idx], memory.rows_of(idx), grad_scale=2.0 / int(idx.numel()))
            trainer.step()
            total += loss / int(idx.numel())  # a batch's MSELoss
        average = float(total) / max(n, 1)
    return average


def optimize_batch(trainer, memory, num_batches, batch_size, generator=None):
    """Trainer.optimize_batch (trainer.py:74-100, RL) with CadrlTrainer: `num_batches` sampled batches, a step each -> the
    mean of the batches' MSELoss."""
    total = torch.zeros((), dtype=torch.float64, device=memory.states.device)
    for _ in range(int(num_batches)):
        inputs, values, rows = memory.sample(int(batch_size), generator, with_rows=True)
        loss, _ = trainer.loss_and_grad(inputs, values, rows, grad_scale=2.0 / int(batch_size))
        trainer.step()
        total += loss / int(batch_size)
    return float(total) / max(int(num_batches), 1)


def _finite(x, what, env):
    """Training stops at the first reward, target or loss that is not finite: nothing of it may reach the weights, and no
    file is written after it.  (A reward is NaN when a collision meets a penalty the env config does not set:
    [reward] collision_penalty_adult / _bicycle / _child / _obstacle; the reference raises there too.)"""
    ok = bool(torch.isfinite(x).all()) if torch.is_tensor(x) else x == x and abs(x) != float("inf")
    if not ok:
        pen = [float(v) for v in env.params.collision_penalty]
        raise FloatingPointError("%s is not finite; training stopped before it reached the weights (collision penalties adult / "
                                 "bicycle / child / obstacle of this env: %s)" % (what, pen))


def run_cadrl_training(env, trainer, actions, gamma, il_steps=0, il_epochs=0, il_learning_rate=0.01, il_safety_space=0.15,
                       rl_learning_rate=0.001, train_iterations=0, steps_per_iteration=1, train_batches=100, batch_size=100,
                       capacity=100000, epsilon_start=0.5, epsilon_end=0.1, epsilon_decay=4000, target_update_interval=50,
                       generator=None, log=None, output_dir=None, checkpoint_interval=0, rank=0, after_il=None):
    """The schedule of rl/train.py:99-260 for CADRL on one rank's env slice (every rank calls it; the gradient is averaged
    over ranks inside CadrlTrainer.step): imitation learning with the robot on ORCA (`il_steps` steps of every env through
    ebc_step_k, then `il_epochs` passes over the memory), then `train_iterations` rounds of [epsilon-greedy rollout of
    `steps_per_iteration` decisions per env with DeviceCadrlPolicy -> `train_batches` optimizer steps on DeviceReplay
    samples -> the deciding blocks re-packed on the device], the target network refreshed every `target_update_interval`
    rounds, epsilon decayed linearly over `epsilon_decay` rounds.  env: BatchedEnv with auto-reset semantics (a scene pool)
    on the trainer's HIP device, rows 13 wide.  output_dir: `il_model.pth` after imitation learning and
    `rl_model_<round>.pth` every `checkpoint_interval` rounds and at the end, in the reference's layout, written by rank 0.
    after_il(hist), when given, runs between the two stages (the replay memory of the imitation stays for the RL rounds).
    A reward, value target or loss that is not finite raises FloatingPointError at once, before an optimizer step sees it.
    Returns a dict of what happened."""
    import torch.distributed as dist
    from .train import DeviceReplay, EpisodeStore, _multi_rank, all_ranks, collect, collect_il
    dev = trainer.device
    if dev.type != "cuda":
        raise NotImplementedError("run_cadrl_training: the rollouts run on a HIP device")
    memory = DeviceReplay(capacity, env.R, env.T, dev)
    hist = {"il_stored": 0, "il_episodes": 0, "il_loss": None, "rl_loss": [], "mean_reward": [], "epsilon": []}

    def save(name):
        if rank == 0 and output_dir:
            os.makedirs(output_dir, exist_ok=True)
            trainer.save(os.path.join(output_dir, name))
    if _multi_rank():  # every replica starts from rank 0's weights
        with torch.no_grad():
            dist.broadcast(trainer.flat, src=0)
        trainer.push_weights()
    red_dev = dev if (_multi_rank() and dist.get_backend() == "nccl") else None
    trainer.set_learning_rate(il_learning_rate)
    if il_steps > 0:
        hist["il_stored"], hist["il_episodes"] = collect_il(env, memory, il_steps, gamma, il_safety_space)
        if il_epochs > 0 and all_ranks(len(memory) > 0, red_dev):
            _finite(memory.values[:len(memory)], "imitation learning: a value target in the replay memory", env)
            hist["il_loss"] = optimize_epoch(trainer, memory, il_epochs, batch_size, generator)
            _finite(hist["il_loss"], "imitation learning: the loss", env)
        save("il_model.pth")
        if log:
            log("imitation learning: %d states of %d episodes, loss %s" % (hist["il_stored"], hist["il_episodes"], hist["il_loss"]))
    if after_il is not None:
        after_il(hist)
    trainer.set_learning_rate(rl_learning_rate)
    # the rollouts decide on the two-layer blocks, packed from the trainer's weights now and re-packed on the device
    # (ebc_mlp2_update) after every round's optimizer steps; the target network likewise at its refresh
    net = CadrlValueNet(trainer.state_dict(), device=dev)
    target_net = CadrlValueNet(trainer.state_dict(), device=dev)  # explorer.update_target_model (train.py:195)
    policy = DeviceCadrlPolicy(net, actions, gamma)
    t_max = int(round(env.params.time_limit / env.params.time_step)) + 2
    store = EpisodeStore(env.E, t_max, env.R, env.T, dev)
    for it in range(int(train_iterations)):
        eps = epsilon_start + (epsilon_end - epsilon_start) / epsilon_decay * it if it < epsilon_decay else epsilon_end
        mean_r = collect(env, policy, target_net, memory, steps_per_iteration, gamma, epsilon=eps, generator=generator, store=store)
        _finite(mean_r, "round %d: the rollout's mean reward" % it, env)
        _finite(memory.values[:len(memory)], "round %d: a value target in the replay memory" % it, env)
        trained = all_ranks(len(memory) > 0, red_dev)
        loss = optimize_batch(trainer, memory, train_batches, batch_size, generator) if trained else float("nan")
        if trained:
            _finite(loss, "round %d: the loss" % it, env)
        net.refresh_native(trainer)
        if (it + 1) % target_update_interval == 0:
            target_net.refresh_native(trainer)
        hist["rl_loss"].append(loss)
        hist["mean_reward"].append(mean_r)
        hist["epsilon"].append(eps)
        if checkpoint_interval and (it + 1) % checkpoint_interval == 0:
            save("rl_model_%d.pth" % (it + 1))
        if log:
            log("iteration %d: epsilon %.3f mean reward %.4f loss %.3e" % (it, eps, mean_r, loss))
    if train_iterations:
        save("rl_model_%d.pth" % train_iterations)
    hist["native_forwards"] = int(net.native_forwards)
    hist["native_refreshes"] = int(net.native_refreshes)
    hist["memory"] = len(memory)
    return hist
