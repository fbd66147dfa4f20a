"""What training a value network on the device shares between CADRL, SARL and LSTM-RL (cadrl_train, sarl_train,
lstm_train): the packed layout's Linear layer, the kernel's network object (GradNet over the ebc_<kind>_net_* entries), the
trainer around ONE flat float32 master copy of the weights (GradTrainer), the optimizer loops of rl/utils/trainer.py
(optimize_epoch, optimize_batch), the states_per_pass choice of the kernels that run a chunk's states in passes, and the
schedule of rl/train.py:99-260 (run_value_training).  The three modules keep what is theirs: the keys and shapes of their
state_dicts, the weights struct of their network object, their kernel's extra outputs, their texts, and how their rollouts
collect.  sail_train is another interface (robot, ob, env-wise masks; a fit loop) and shares nothing here."""
import collections
import ctypes as C
import os

import torch

PASS_SIZES = (4, 2, 1)  # EbcSarlGradArgs.states_per_pass / EbcLstmGradArgs.states_per_pass: a chunk's states, that many at a time


def pad4(n):
    return (int(n) + 3) & ~3


def linear_views(out, flat, at, key, k, o):
    """A Linear layer of k inputs and o units at flat[at:], W[k][o padded to a multiple of 4] then the bias [o padded]: its
    views in torch's shapes into out[key + ".weight"] ([o, k]) and out[key + ".bias"] ([o]) -> where the next layer starts."""
    op = pad4(o)
    out[key + ".weight"] = flat[at:at + k * op].view(k, op)[:, :o].t()
    out[key + ".bias"] = flat[at + k * op:at + (k + 1) * op][:o]
    return at + (k + 1) * op


def pack_into(sd, out, floats, like, views):
    """A state_dict -> the packed image, flat float32: into `out` when given, else a new tensor of `floats` on `like`'s
    device; views(flat): the state_dict's keys -> their views into flat.  Pad entries are 0."""
    if out is None:
        out = torch.zeros(floats, dtype=torch.float32, device=like.device)
    else:
        out.zero_()
    with torch.no_grad():
        for key, v in views(out).items():
            v.copy_(sd[key])
    return out


def live_states(B, R, n_valid, mask, device):
    """live as a bool tensor [B]: mask != 0 and at least one row."""
    w = torch.ones(B, dtype=torch.bool, device=device)
    if n_valid is not None:
        w = w & (n_valid.to(device) >= 1)
    if mask is not None:
        w = w & (mask.to(device) != 0)
    return w


def checked_states_per_pass(value, who):
    """A trainer's states_per_pass: None (the whole chunk at once, the kernel's default call), "auto", 1, 2 or 4."""
    if value is None or value == "auto" or (type(value) is int and value in PASS_SIZES):
        return value
    raise ValueError("%s: states_per_pass is None, 'auto', 1, 2 or 4, got %r" % (who, value))


def pick_states_per_pass(R, whole_chunk, limits):
    """What "auto" passes to the kernel for states of R rows.  whole_chunk: the largest R of the default call
    (grad_max_rows()); limits: {S: grad_max_rows(S)} for S in PASS_SIZES.  0 (the default call) where the whole chunk
    fits, else the largest S whose limit holds R; past every limit 1, which the kernel then refuses by R, S and limit."""
    if R <= whole_chunk:
        return 0
    for S in PASS_SIZES:
        if R <= limits[S]:
            return S
    return PASS_SIZES[-1]


class PassChoice(object):
    """A trainer's states_per_pass over its network object (SarlNet / LstmNet): what each call passes and the most rows
    the trainer takes.  The limits are asked of the network once."""

    def __init__(self, net, setting):
        self.setting = setting
        self.whole_chunk = net.grad_max_rows()
        self.limits = {S: net.grad_max_rows(S) for S in PASS_SIZES}

    def of(self, R):
        if self.setting is None:
            return 0
        return pick_states_per_pass(R, self.whole_chunk, self.limits) if self.setting == "auto" else self.setting

    def max_rows(self):
        if self.setting is None:
            return self.whole_chunk
        return max(self.whole_chunk, *self.limits.values()) if self.setting == "auto" else self.limits[self.setting]


class GradNet(object):
    """The kernel's network object behind the entries ebc_<kind>_net_* and ebc_<kind>_grad: the packed image of a
    state_dict in device memory.  A subclass names its KIND and its ARGS struct, creates the handle self._h in its
    __init__ (self._L the library) and gives `grad` its own signature over _grad."""
    KIND = None  # "cadrl", "sarl", "lstm"
    ARGS = None  # _abi.Ebc<Kind>GradArgs

    def _entry(self, name):
        return getattr(self._L, "ebc_%s_%s" % (self.KIND, name))

    def packed_floats(self):
        from . import _capi
        n = C.c_int64()
        _capi.check(self._entry("net_packed_floats")(self._h, C.byref(n)))
        return int(n.value)

    def grad_max_rows(self, states_per_pass=0):
        """The largest R the kernel takes for this network: a chunk's activations (states_per_pass 4, 2, 1: those of that
        many states) fit a workgroup's LDS.  Of the kinds whose kernel has such a limit: SARL and LSTM-RL."""
        from . import _capi
        n = C.c_int()
        if states_per_pass == 0:
            _capi.check(self._entry("net_grad_max_rows")(self._h, C.byref(n)))
        else:
            _capi.check(self._entry("net_grad_max_rows_at")(self._h, int(states_per_pass), C.byref(n)))
        return int(n.value)

    def get_packed(self, out):
        from . import _capi
        assert out.dtype == torch.float32 and out.is_contiguous() and out.is_cuda and out.numel() == self.packed_floats()
        _capi.check(self._entry("net_get_packed")(self._h, torch.cuda.current_stream(out.device).cuda_stream, out.data_ptr()))
        return out

    def set_packed(self, flat):
        from . import _capi
        assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.is_cuda and flat.numel() == self.packed_floats()
        _capi.check(self._entry("net_set_packed")(self._h, torch.cuda.current_stream(flat.device).cuda_stream, flat.data_ptr()))

    def _grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid, mask, value, extra, T=None, states_per_pass=None):
        """One ebc_<kind>_grad on the current stream.  extra: the kernel's own output as (name, tensor or None, dtype,
        numel); T: the width the args declare when it is not the rows'; states_per_pass: None where the args have none."""
        from . import _capi
        B, R, Tr = (int(x) for x in rows.shape)
        a = self.ARGS()
        a.struct_size = C.sizeof(a)
        a.B, a.R, a.T, a.grad_scale = B, R, Tr if T is None else int(T), float(grad_scale)
        if states_per_pass is not None:
            a.states_per_pass = int(states_per_pass)
        for name, t, dtype, numel in (("rows", rows, torch.float32, B * R * Tr), ("target", target, torch.float32, B),
                                      ("n_valid", n_valid, torch.int64, B), ("sample_mask", mask, torch.uint8, B),
                                      ("grad", grad, torch.float32, self.packed_floats()), ("loss_sum", loss_sum, torch.float64, 1),
                                      ("count", count, torch.int64, 1), ("value", value, torch.float32, B), extra):
            if t is None:
                continue
            assert t.dtype == dtype and t.is_contiguous() and t.is_cuda and t.numel() == numel, name
            setattr(a, name, t.data_ptr())
        _capi.check(self._entry("grad")(self._h, torch.cuda.current_stream(rows.device).cuda_stream, C.addressof(a)))

    def __del__(self):
        try:
            self._entry("net_destroy")(self._h)
        except Exception:
            pass


class GradTrainer(object):
    """The trainer around ONE flat float32 tensor in the kernel's packed layout, the master copy of the weights: the
    kernel (or, with native=False and on every CPU device, torch's autograd on the network's module) writes its .grad, a
    torch optimizer steps it, the kernel's network object gets the result back.  A subclass supplies:
      NAME, EXTRA, OTHER_SHAPE   its name and its kernel's extra output in the texts; load_state_dict's refusal
      _configure(sd, **options)  reads the state_dict's shape into self.widths (...) and checks the options
      _shape_of(sd), _shape()    a state_dict's shape and this trainer's, as load_state_dict compares them
      _pack(sd, out=None)        the module's pack_state_dict
      _views(flat)               the reference's keys -> views into a flat packed tensor
      _module_of(sd)             the autograd path's module; _forward(x, n_valid) its values [B]; _param_key(name) the
                                 reference's key of a parameter of it
      _new_net(sd, index)        the kernel's network object; _grad_options(R) its grad's keywords for states of R rows"""
    NAME = EXTRA = OTHER_SHAPE = None

    def __init__(self, module_or_state_dict, device, optimizer, lr, native, **options):
        sd = module_or_state_dict.state_dict() if isinstance(module_or_state_dict, torch.nn.Module) else module_or_state_dict
        sd = collections.OrderedDict((k, v.detach().to("cpu", torch.float32)) for k, v in sd.items())
        self.device = torch.device(device)
        self._configure(sd, **options)
        self.native = (self.device.type == "cuda") if native is None else bool(native)
        if self.native and self.device.type != "cuda":
            raise NotImplementedError("%s(native=True) needs a HIP device: the kernel has no CPU form" % self.NAME)
        self.flat = self._pack(sd).to(self.device).requires_grad_(True)
        self.flat.grad = torch.zeros_like(self.flat)
        self._optimizer_spec = optimizer
        self.set_learning_rate(lr)
        self.module = self._module_of(sd).to(self.device)  # the autograd path's
        self.net = None
        if self.native:
            self.net = self._new_net(sd, self.device.index if self.device.index is not None else torch.cuda.current_device())

    _param_key = staticmethod(lambda name: name)

    def _forward(self, x, n_valid):
        return self.module(x, n_valid)

    def _grad_options(self, R):
        return {}

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
        """The current weights under the reference's keys, fresh contiguous tensors on the CPU."""
        return collections.OrderedDict((k, v.clone().contiguous()) for k, v in self._views(self.flat.detach().cpu()).items())

    def device_state_dict(self):
        """The reference's keys as views into the master copy on its device (no copy): what the deciding network's
        refresh_native / refresh_from reads."""
        return self._views(self.flat.detach())

    def save(self, path):
        """The current weights as a file torch.save wrote: loads into the network's module and the reference's
        ValueNetwork with strict=True."""
        torch.save(self.state_dict(), path)

    def load_state_dict(self, sd):
        if self._shape_of(sd) != self._shape():
            raise ValueError("%s.load_state_dict: %s" % (self.NAME, self.OTHER_SHAPE))
        with torch.no_grad():
            self._pack({k: v.to(self.device, torch.float32) for k, v in sd.items()}, out=self.flat)
        self.push_weights()

    def push_weights(self):
        """The master copy into the kernel's network object (ebc_<kind>_net_set_packed on the current stream)."""
        if self.net is not None:
            self.net.set_packed(self.flat.detach())

    def _module_params(self):
        return {self._param_key(k): p for k, p in self.module.named_parameters()}

    def _load_module(self):
        with torch.no_grad():
            params = self._module_params()
            for key, v in self._views(self.flat.detach()).items():
                params[key].copy_(v)

    # ------------------------------------------------------------------ loss and gradient
    def _loss_and_grad(self, rows, target, n_valid, mask, grad_scale, value, extra):
        """loss_and_grad of the subclass, whose docstring says what goes in and out; extra: its kernel's own output."""
        rows, target = rows.to(self.device, torch.float32).contiguous(), target.to(self.device, torch.float32).reshape(-1).contiguous()
        B, R, T = (int(x) for x in rows.shape)
        if T != self.widths[0]:
            raise ValueError("%s: rows are %d wide, the network takes %d" % (self.NAME, T, self.widths[0]))
        live = None
        if grad_scale is None:
            live = live_states(B, R, n_valid, mask, self.device)
            grad_scale = 2.0 / max(int(live.sum()), 1)
        if self.native:
            loss = torch.empty((), dtype=torch.float64, device=self.device)
            count = torch.empty((), dtype=torch.int64, device=self.device)
            nv = None if n_valid is None else n_valid.to(device=self.device, dtype=torch.int64).contiguous()
            mk = None if mask is None else mask.to(device=self.device).to(torch.uint8).contiguous()
            self.net.grad(rows, target, self.flat.grad, loss, count, grad_scale, nv, mk, value, extra, **self._grad_options(R))
            return loss, count
        if value is not None or extra is not None:
            raise NotImplementedError("%s(native=False): `value` and `%s` are the kernel's outputs" % (self.NAME, self.EXTRA))
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
        with torch.enable_grad():
            d = self._forward(x, nv) - target[idx]
            (0.5 * float(grad_scale) * (d * d).sum()).backward()
        self._pack({k: p.grad for k, p in self._module_params().items()}, out=self.flat.grad)
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


class PassTrainer(GradTrainer):
    """A GradTrainer whose kernel runs a chunk's states in passes (SARL, LSTM-RL): states_per_pass and the row limits."""

    def _new_net(self, sd, index):
        net = self._new_pass_net(sd, index)
        self.passes = PassChoice(net, self.states_per_pass)
        return net

    def _grad_options(self, R):
        return {"states_per_pass": self.passes.of(R)}

    def grad_max_rows(self):
        """The most rows per state the native path takes with this trainer's states_per_pass."""
        return self.passes.max_rows()


def optimize_epoch(trainer, memory, num_epochs, batch_size, generator=None):
    """Trainer.optimize_epoch (trainer.py:45-72, imitation learning) with a GradTrainer: `num_epochs` shuffled passes over
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
    """Trainer.optimize_batch (trainer.py:74-100, RL) with a GradTrainer: `num_batches` sampled batches, a step each -> the
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


def run_value_training(env, trainer, gamma, width, new_net, new_policy, refresh, il_options, collect_options, il_steps, il_epochs,
                       il_learning_rate, il_safety_space, rl_learning_rate, train_iterations, steps_per_iteration, train_batches,
                       batch_size, capacity, epsilon_start, epsilon_end, epsilon_decay, target_update_interval, generator, log,
                       output_dir, checkpoint_interval, rank, after_il):
    """The schedule of rl/train.py:99-260 behind run_cadrl_training, run_sarl_training and run_lstm_training, whose
    docstrings say what it does and whose checks have passed.  width: of the stored states' rows; new_net(): a deciding
    network from the trainer's weights (called twice: the second is the target network); new_policy(net): the policy that
    decides on it; refresh(net): the trainer's weights into it on the device; il_options / collect_options: the keywords
    collect_il and collect take beside the schedule's own."""
    import torch.distributed as dist
    from .train import DeviceReplay, EpisodeStore, _multi_rank, all_ranks, collect, collect_il
    dev = trainer.device
    memory = DeviceReplay(capacity, env.R, width, dev)
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
        hist["il_stored"], hist["il_episodes"] = collect_il(env, memory, il_steps, gamma, il_safety_space, **il_options)
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
    # the rollouts decide on a network packed from the trainer's weights now and refreshed on the device after every
    # round's optimizer steps; the target network likewise at its refresh
    net = new_net()
    target_net = new_net()  # explorer.update_target_model (train.py:195)
    policy = new_policy(net)
    t_max = int(round(env.params.time_limit / env.params.time_step)) + 2
    store = EpisodeStore(env.E, t_max, env.R, width, dev)
    for it in range(int(train_iterations)):
        eps = epsilon_start + (epsilon_end - epsilon_start) / epsilon_decay * it if it < epsilon_decay else epsilon_end
        mean_r = collect(env, policy, target_net, memory, steps_per_iteration, gamma, epsilon=eps, generator=generator, store=store,
                         **collect_options)
        _finite(mean_r, "round %d: the rollout's mean reward" % it, env)
        _finite(memory.values[:len(memory)], "round %d: a value target in the replay memory" % it, env)
        trained = all_ranks(len(memory) > 0, red_dev)
        loss = optimize_batch(trainer, memory, train_batches, batch_size, generator) if trained else float("nan")
        if trained:
            _finite(loss, "round %d: the loss" % it, env)
        refresh(net)
        if (it + 1) % target_update_interval == 0:
            refresh(target_net)
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
