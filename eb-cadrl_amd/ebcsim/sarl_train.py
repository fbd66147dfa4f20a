"""Training the SARL value network on the device: rollouts -> the fused forward + backward kernel (ebc_sarl_grad,
csrc/ebc_sarl_grad.h) -> a torch optimizer -> a state_dict in the reference's ValueNetwork layout (mlp1.0.weight ...
mlp3.6.bias) that tools/evaluate.py loads.

SarlTrainer keeps ONE flat float32 tensor in the kernel's packed layout (csrc/ebc_sarl_grad_rule.h: the eleven layers in
the order mlp1, mlp2, attention, mlp3; per layer W[k][units padded to a multiple of 4], then the bias, pad entries 0) as
the master copy of the weights.  The kernel writes its .grad, a torch optimizer steps it, ebc_sarl_net_set_packed hands the
result back to the kernel's network object and SarlValueNet.refresh_from hands it to the matrix-core blocks that decide.
native=False (and every CPU device) computes the same loss and gradient with torch's autograd on SarlModule: the
comparison path, and what the CPU tests drive.  ebcsim.train.DataParallelTrainer and run_training stay what they were.

The loss is the reference's (rl/utils/trainer.py:74-100): the mean squared error between the network's value of a state
and its target.  optimize_epoch and optimize_batch are cadrl_train's (they take any trainer with this interface);
run_sarl_training is the schedule of rl/train.py:99-260 on the generic pieces of ebcsim.train with this trainer in the
optimizer's place and DeviceSarlPolicy deciding.

OM-SARL (om_width = W > 0, run_sarl_training(om=spec)): mlp1's first layer takes T + W inputs, the kernel's network is
ebc_sarl_net_create_om's, the stored states are the wide ones (BatchedEnv.observe_wide_device, ebc_step_k_om) and
DeviceSarlPolicy(om=spec) decides.  The width of the maps is not in a state_dict (only T + W is): it is given explicitly."""
import collections
import ctypes as C
import os

import torch

from . import _abi
from .cadrl_train import _finite, live_states, optimize_batch, optimize_epoch, pad4  # noqa: F401 (re-exported)
from .sarl import DeviceSarlPolicy, SarlValueNet
from .train import SarlModule

LAYER_KEYS = ("mlp1.0", "mlp1.2", "mlp2.0", "mlp2.2", "attention.0", "attention.2", "attention.4", "mlp3.0", "mlp3.2", "mlp3.4",
              "mlp3.6")
STACKS = (("mlp1", 2), ("mlp2", 2), ("attention", 3), ("mlp3", 4))
MAX_IN, MAX_WIDTH = 64, 256  # csrc/ebc_sarl_grad_rule.h
MAX_OM, MAX_WIDE = 192, 224  # the same: the widest map behind a row, the widest row with its map
PASS_SIZES = (4, 2, 1)  # EbcSarlGradArgs.states_per_pass / EbcLstmGradArgs.states_per_pass: a chunk's states, that many at a time


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


def _stack_keys(sd):
    out = collections.OrderedDict()
    for name, _ in STACKS:
        out[name] = ["%s.%d" % (name, i) for i in sorted({int(k.split(".")[1]) for k in sd if k.startswith(name + ".") and k.endswith(".weight")})]
    return out


def widths_of(sd):
    """[row width, units of mlp1 (2), mlp2 (2), attention (3), mlp3 (4)] of a state_dict with the reference's keys."""
    keys = [k for ks in _stack_keys(sd).values() for k in ks]
    if keys != list(LAYER_KEYS):
        raise NotImplementedError("SARL training: mlp1 / mlp2 / attention / mlp3 of 2 / 2 / 3 / 4 Linear layers (%s), got %s"
                                  % (", ".join(LAYER_KEYS), keys))
    return [int(sd["mlp1.0.weight"].shape[1])] + [int(sd[k + ".weight"].shape[0]) for k in LAYER_KEYS]


def shape_of(sd):
    """(widths, self_state_dim, with_global_state) of a state_dict: attention's layer 0 takes mlp1's output once or twice,
    mlp3's layer 0 the self state beside mlp2's output."""
    w = widths_of(sd)
    att_in, H = int(sd["attention.0.weight"].shape[1]), w[2]
    if att_in not in (H, 2 * H):
        raise ValueError("attention.0 takes %d inputs, mlp1 gives %d" % (att_in, H))
    return w, int(sd["mlp3.0.weight"].shape[1]) - w[4], att_in == 2 * H


def layer_inputs(widths, self_state_dim=6, with_global_state=True):
    """The inputs K of the eleven layers."""
    K = list(widths[:-1])
    K[4] = widths[2] * (2 if with_global_state else 1)
    K[7] = int(self_state_dim) + widths[4]
    return K


def packed_floats(widths, self_state_dim=6, with_global_state=True):
    return sum((k + 1) * pad4(o) for k, o in zip(layer_inputs(widths, self_state_dim, with_global_state), widths[1:]))


def _layer_views(flat, widths, self_state_dim, with_global_state):
    """Per layer (W view [out, in], bias view [out]) into a flat packed tensor."""
    out, at = [], 0
    for k, o in zip(layer_inputs(widths, self_state_dim, with_global_state), widths[1:]):
        op = pad4(o)
        out.append((flat[at:at + k * op].view(k, op)[:, :o].t(), flat[at + k * op:at + (k + 1) * op][:o]))
        at += (k + 1) * op
    return out


def pack_state_dict(sd, out=None):
    """A state_dict of the reference's keys -> the packed image, flat float32 (into `out` when given)."""
    widths, S, glob = shape_of(sd)
    if out is None:
        out = torch.zeros(packed_floats(widths, S, glob), dtype=torch.float32, device=sd["mlp1.0.weight"].device)
    else:
        out.zero_()
    with torch.no_grad():
        for key, (w, b) in zip(LAYER_KEYS, _layer_views(out, widths, S, glob)):
            w.copy_(sd[key + ".weight"])
            b.copy_(sd[key + ".bias"])
    return out


def unpack_to_state_dict(flat, widths, self_state_dim=6, with_global_state=True):
    """The packed image -> an ordered state_dict with SarlModule's (the reference's) keys, fresh contiguous tensors."""
    sd = collections.OrderedDict()
    for key, (w, b) in zip(LAYER_KEYS, _layer_views(flat.detach(), widths, self_state_dim, with_global_state)):
        sd[key + ".weight"] = w.clone().contiguous()
        sd[key + ".bias"] = b.clone().contiguous()
    return sd


def module_of(sd):
    """A SarlModule of the state_dict's shape with its weights."""
    w, S, glob = shape_of(sd)
    m = SarlModule(w[0], w[1:3], w[3:5], w[8:12], w[5:8], with_global_state=glob, self_state_dim=S)
    m.load_state_dict({k: sd[k] for k in m.state_dict()})
    return m


class SarlNet(object):
    """The kernel's network object (ebc_sarl_net_*): the packed image of a state_dict in device memory."""

    def __init__(self, sd, device_index, widths=None, self_state_dim=None, with_global_state=None, stack_layers=None, om_width=None):
        """widths / self_state_dim / with_global_state / stack_layers override what the state_dict says (the tests of the
        entry's refusals).  om_width: None = ebc_sarl_net_create; an int W = ebc_sarl_net_create_om, whose rotated width
        is mlp1.0.weight.shape[1] - W (widths[0], when given, is that rotated width)."""
        from . import _capi
        self._L = _capi.lib()
        keys = [k for ks in _stack_keys(sd).values() for k in ks]
        host = [(sd[k + ".weight"].detach().to("cpu", torch.float32).contiguous().numpy(),
                 sd[k + ".bias"].detach().to("cpu", torch.float32).contiguous().numpy()) for k in keys]
        self._keep = host
        counts = stack_layers if stack_layers is not None else [len(ks) for ks in _stack_keys(sd).values()]
        if len(keys) > _abi.SARL_NET_MAX_LAYERS:
            raise NotImplementedError("SARL training: more than %d Linear layers" % _abi.SARL_NET_MAX_LAYERS)
        w = _abi.EbcSarlNetWeights()
        w.struct_size = C.sizeof(w)
        w.n_mlp1, w.n_mlp2, w.n_attention, w.n_mlp3 = (int(c) for c in counts)
        H = int(host[counts[0] - 1][0].shape[0]) if counts[0] >= 1 else 0
        att_in = int(sd["attention.0.weight"].shape[1])
        w.with_global_state = int(att_in == 2 * H) if with_global_state is None else int(with_global_state)
        units = [int(a.shape[0]) for a, _ in host] if widths is None else list(widths[1:])
        w.input_dim = int(host[0][0].shape[1]) - int(om_width or 0) if widths is None else int(widths[0])
        F = units[counts[0] + counts[1] - 1]
        w.self_state_dim = int(sd["mlp3.0.weight"].shape[1]) - F if self_state_dim is None else int(self_state_dim)
        for i, v in enumerate(units):
            w.widths[i] = v
        for i, (a, b) in enumerate(host):
            w.weight[i], w.bias[i] = a.ctypes.data, b.ctypes.data
        self._h = C.c_void_p()
        if om_width is None:
            _capi.check(self._L.ebc_sarl_net_create(C.addressof(w), int(device_index), C.byref(self._h)))
        else:
            _capi.check(self._L.ebc_sarl_net_create_om(C.addressof(w), int(om_width), int(device_index), C.byref(self._h)))
        self.om_width = int(om_width or 0)
        self.widths = [w.input_dim + self.om_width] + units  # [0]: the rows ebc_sarl_grad takes

    def packed_floats(self):
        from . import _capi
        n = C.c_int64()
        _capi.check(self._L.ebc_sarl_net_packed_floats(self._h, C.byref(n)))
        return int(n.value)

    def grad_max_rows(self, states_per_pass=0):
        """The largest R ebc_sarl_grad takes for this network: a chunk's activations (states_per_pass 4, 2, 1: those of
        that many states) fit a workgroup's LDS."""
        from . import _capi
        n = C.c_int()
        if states_per_pass == 0:
            _capi.check(self._L.ebc_sarl_net_grad_max_rows(self._h, C.byref(n)))
        else:
            _capi.check(self._L.ebc_sarl_net_grad_max_rows_at(self._h, int(states_per_pass), C.byref(n)))
        return int(n.value)

    def get_packed(self, out):
        from . import _capi
        assert out.dtype == torch.float32 and out.is_contiguous() and out.is_cuda and out.numel() == self.packed_floats()
        _capi.check(self._L.ebc_sarl_net_get_packed(self._h, torch.cuda.current_stream(out.device).cuda_stream, out.data_ptr()))
        return out

    def set_packed(self, flat):
        from . import _capi
        assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.is_cuda and flat.numel() == self.packed_floats()
        _capi.check(self._L.ebc_sarl_net_set_packed(self._h, torch.cuda.current_stream(flat.device).cuda_stream, flat.data_ptr()))

    def grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, attention=None, T=None,
             states_per_pass=0):
        """One ebc_sarl_grad on the current stream: rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None,
        mask [B] uint8 or None -> grad [packed floats], loss_sum 0-d float64, count 0-d int64, value [B] float32 and
        attention [B, R] float32 when given; every tensor contiguous on the network's device.  states_per_pass: 0 = the
        whole chunk at once; 4, 2, 1 = that many of a chunk's states at a time (more rows fit, the same bytes)."""
        from . import _capi
        B, R, Tr = (int(x) for x in rows.shape)
        a = _abi.EbcSarlGradArgs()
        a.struct_size = C.sizeof(a)
        a.B, a.R, a.T, a.grad_scale = B, R, Tr if T is None else int(T), float(grad_scale)
        a.states_per_pass = int(states_per_pass)
        for name, t, dtype, numel in (("rows", rows, torch.float32, B * R * Tr), ("target", target, torch.float32, B),
                                      ("n_valid", n_valid, torch.int64, B), ("sample_mask", mask, torch.uint8, B),
                                      ("grad", grad, torch.float32, self.packed_floats()), ("loss_sum", loss_sum, torch.float64, 1),
                                      ("count", count, torch.int64, 1), ("value", value, torch.float32, B),
                                      ("attention", attention, torch.float32, B * R)):
            if t is None:
                continue
            assert t.dtype == dtype and t.is_contiguous() and t.is_cuda and t.numel() == numel, name
            setattr(a, name, t.data_ptr())
        _capi.check(self._L.ebc_sarl_grad(self._h, torch.cuda.current_stream(rows.device).cuda_stream, C.addressof(a)))

    def __del__(self):
        try:
            self._L.ebc_sarl_net_destroy(self._h)
        except Exception:
            pass


class SarlTrainer(object):
    """module_or_state_dict: a SarlModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "sgd" (momentum 0.9), "adam" (rl/utils/trainer.py:24-45) or a callable params -> torch optimizer.  native: the kernel
    (HIP devices only; the default there) or torch autograd of SarlModule.  om_width: the W of OM-SARL's maps; the
    network's mlp1.0 then takes T + W inputs, T = widths[0] - W the rotated width (1 .. 64), W <= 192, T + W <= 224.
    states_per_pass (native only; native=False ignores it): None = the kernel's default call, the whole chunk of 4 states
    at once; 1, 2, 4 = that many states at a time, which takes more rows per state (SarlNet.grad_max_rows(S)) and gives
    the same bytes; "auto" = per call the default call where the batch's R fits it, else the largest pass that holds R."""

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None, om_width=0, states_per_pass=None):
        sd = module_or_state_dict.state_dict() if isinstance(module_or_state_dict, torch.nn.Module) else module_or_state_dict
        sd = collections.OrderedDict((k, v.detach().to("cpu", torch.float32)) for k, v in sd.items())
        self.device = torch.device(device)
        self.widths, self.self_state_dim, self.with_global_state = shape_of(sd)
        self.om_width = int(om_width)
        self.states_per_pass = checked_states_per_pass(states_per_pass, "SarlTrainer")
        if not 0 <= self.om_width <= MAX_OM:
            raise NotImplementedError("SarlTrainer: om_width %d outside 0 .. %d" % (self.om_width, MAX_OM))
        if self.widths[0] - self.om_width < 1:
            raise ValueError("SarlTrainer: om_width %d leaves no rotated columns of mlp1.0's %d inputs" % (self.om_width, self.widths[0]))
        if self.om_width and self.widths[0] > MAX_WIDE:
            raise NotImplementedError("SarlTrainer: T + om_width = %d columns, the gradient takes up to %d" % (self.widths[0], MAX_WIDE))
        self.native = (self.device.type == "cuda") if native is None else bool(native)
        if self.native and self.device.type != "cuda":
            raise NotImplementedError("SarlTrainer(native=True) needs a HIP device: the kernel has no CPU form")
        self.flat = pack_state_dict(sd).to(self.device).requires_grad_(True)
        self.flat.grad = torch.zeros_like(self.flat)
        self._optimizer_spec = optimizer
        self.set_learning_rate(lr)
        self.module = module_of(sd).to(self.device)  # the autograd path's
        self.net = None
        if self.native:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.net = SarlNet(sd, idx, om_width=self.om_width or None)
            self.passes = PassChoice(self.net, self.states_per_pass)

    def grad_max_rows(self):
        """The most rows per state the native path takes with this trainer's states_per_pass."""
        return self.passes.max_rows()

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

    def _views(self, flat):
        return _layer_views(flat, self.widths, self.self_state_dim, self.with_global_state)

    # ------------------------------------------------------------------ weights
    def state_dict(self):
        return unpack_to_state_dict(self.flat.detach().cpu(), self.widths, self.self_state_dim, self.with_global_state)

    def device_state_dict(self):
        """The reference's keys as views into the master copy on its device (no copy): what SarlValueNet.refresh_from reads."""
        sd = collections.OrderedDict()
        for key, (w, b) in zip(LAYER_KEYS, self._views(self.flat.detach())):
            sd[key + ".weight"], sd[key + ".bias"] = w, b
        return sd

    def save(self, path):
        """The current weights as a file torch.save wrote: loads into SarlModule and the reference's ValueNetwork with
        strict=True."""
        torch.save(self.state_dict(), path)

    def load_state_dict(self, sd):
        if shape_of(sd) != (self.widths, self.self_state_dim, self.with_global_state):
            raise ValueError("SarlTrainer.load_state_dict: another network shape")
        with torch.no_grad():
            pack_state_dict({k: v.to(self.device, torch.float32) for k, v in sd.items()}, out=self.flat)
        self.push_weights()

    def push_weights(self):
        """The master copy into the kernel's network object (ebc_sarl_net_set_packed on the current stream)."""
        if self.net is not None:
            self.net.set_packed(self.flat.detach())

    def _load_module(self):
        with torch.no_grad():
            params = self.module.reference_state_dict()
            for key, (w, b) in zip(LAYER_KEYS, self._views(self.flat.detach())):
                params[key + ".weight"].copy_(w)
                params[key + ".bias"].copy_(b)

    # ------------------------------------------------------------------ loss and gradient
    def loss_and_grad(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, attention=None):
        """rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None, mask [B] uint8 / bool or None, on the
        trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64) there; .grad of the master copy holds
        d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 2 / count, torch's MSELoss over the live states (this
        reads the count back).  value [B] float32 / attention [B, R] float32, when given, receive the states' values and
        softmax weights (native only)."""
        rows, target = rows.to(self.device, torch.float32).contiguous(), target.to(self.device, torch.float32).reshape(-1).contiguous()
        B, R, T = (int(x) for x in rows.shape)
        if T != self.widths[0]:
            raise ValueError("SarlTrainer: rows are %d wide, the network takes %d" % (T, self.widths[0]))
        live = None
        if grad_scale is None:
            live = live_states(B, R, n_valid, mask, self.device)
            grad_scale = 2.0 / max(int(live.sum()), 1)
        if self.native:
            loss = torch.empty((), dtype=torch.float64, device=self.device)
            count = torch.empty((), dtype=torch.int64, device=self.device)
            nv = None if n_valid is None else n_valid.to(device=self.device, dtype=torch.int64).contiguous()
            mk = None if mask is None else mask.to(device=self.device).to(torch.uint8).contiguous()
            self.net.grad(rows, target, self.flat.grad, loss, count, grad_scale, nv, mk, value, attention, states_per_pass=self.passes.of(R))
            return loss, count
        if value is not None or attention is not None:
            raise NotImplementedError("SarlTrainer(native=False): `value` and `attention` are the kernel's outputs")
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
            # rows past a state's own are never read by the kernel; autograd multiplies their (zero) weights with them, so
            # a NaN there must not be an input
            nv = n_valid.to(self.device)[idx].clamp(max=R)
            x = torch.where((torch.arange(R, device=self.device)[None, :] < nv[:, None])[:, :, None], x, torch.zeros_like(x))
        with torch.enable_grad():
            out = self.module(x, nv)
            d = out - target[idx]
            (0.5 * float(grad_scale) * (d * d).sum()).backward()
        pack_state_dict({SarlModule._ref_name(k): p.grad for k, p in self.module.named_parameters()}, out=self.flat.grad)
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


def run_sarl_training(env, trainer, actions, gamma, il_steps=0, il_epochs=0, il_learning_rate=0.01, il_safety_space=0.15,
                      rl_learning_rate=0.001, train_iterations=0, steps_per_iteration=1, train_batches=100, batch_size=100,
                      capacity=100000, epsilon_start=0.5, epsilon_end=0.1, epsilon_decay=4000, target_update_interval=50,
                      generator=None, log=None, output_dir=None, checkpoint_interval=0, rank=0, after_il=None, om=None):
    """The schedule of cadrl_train.run_cadrl_training (rl/train.py:99-260) for SARL on one rank's env slice: imitation
    learning with the robot on ORCA, then `train_iterations` rounds of [epsilon-greedy rollout with DeviceSarlPolicy ->
    `train_batches` optimizer steps on DeviceReplay samples -> the deciding network's tensors and matrix-core blocks
    refreshed from the trainer on the device], the target network refreshed every `target_update_interval` rounds.
    env: BatchedEnv with auto-reset semantics (a scene pool) on the trainer's HIP device.  output_dir: `il_model.pth`
    after imitation learning and `rl_model_<round>.pth` every `checkpoint_interval` rounds and at the end.  A reward,
    value target or loss that is not finite raises FloatingPointError at once, before an optimizer step sees it.
    om (an occupancy.OccupancySpec): OM-SARL.  The trainer's network takes T + om.width columns (SarlTrainer(om_width=
    om.width)), the replay and the episode store hold the wide states, collect_il and collect store them (ebc_step_k_om,
    ebc_observe_wide) and DeviceSarlPolicy(om=om) decides.
    Returns a dict of what happened."""
    import torch.distributed as dist
    from .train import DeviceReplay, EpisodeStore, _multi_rank, all_ranks, collect, collect_il
    dev = trainer.device
    if dev.type != "cuda":
        raise NotImplementedError("run_sarl_training: the rollouts run on a HIP device")
    W = 0 if om is None else int(om.width)
    if env.T + W != trainer.widths[0] or W != getattr(trainer, "om_width", 0):
        raise NotImplementedError("run_sarl_training: the env's rows are %d wide and the occupancy maps %d, the network takes %d "
                                  "(%d of them maps)" % (env.T, W, trainer.widths[0], getattr(trainer, "om_width", 0)))
    if trainer.native and env.R > trainer.grad_max_rows():
        raise NotImplementedError("run_sarl_training: %d rows per state, ebc_sarl_grad takes %d for this network; use native=False"
                                  % (env.R, trainer.grad_max_rows()))
    memory = DeviceReplay(capacity, env.R, env.T + W, dev)
    om_kw = {} if om is None else {"om": om}  # without maps: the calls as they were
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
        hist["il_stored"], hist["il_episodes"] = collect_il(env, memory, il_steps, gamma, il_safety_space, **om_kw)
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
    kw = dict(device=dev, with_global_state=trainer.with_global_state, self_state_dim=trainer.self_state_dim)
    net = SarlValueNet(trainer.state_dict(), **kw)
    target_net = SarlValueNet(trainer.state_dict(), **kw)  # explorer.update_target_model (train.py:195)
    policy = DeviceSarlPolicy(net, actions, gamma, **om_kw)
    t_max = int(round(env.params.time_limit / env.params.time_step)) + 2
    store = EpisodeStore(env.E, t_max, env.R, env.T + W, dev)
    for it in range(int(train_iterations)):
        eps = epsilon_start + (epsilon_end - epsilon_start) / epsilon_decay * it if it < epsilon_decay else epsilon_end
        mean_r = collect(env, policy, target_net, memory, steps_per_iteration, gamma, epsilon=eps, generator=generator, store=store, **om_kw)
        _finite(mean_r, "round %d: the rollout's mean reward" % it, env)
        _finite(memory.values[:len(memory)], "round %d: a value target in the replay memory" % it, env)
        trained = all_ranks(len(memory) > 0, red_dev)
        loss = optimize_batch(trainer, memory, train_batches, batch_size, generator) if trained else float("nan")
        if trained:
            _finite(loss, "round %d: the loss" % it, env)
        net.refresh_from(trainer)
        if (it + 1) % target_update_interval == 0:
            target_net.refresh_from(trainer)
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
