"""Training the SARL value network on the device: rollouts -> the fused forward + backward kernel (ebc_sarl_grad,
csrc/ebc_sarl_grad.h) -> a torch optimizer -> a state_dict in the reference's ValueNetwork layout (mlp1.0.weight ...
mlp3.6.bias) that tools/evaluate.py loads.

SarlTrainer keeps ONE flat float32 tensor in the kernel's packed layout (csrc/ebc_sarl_grad_rule.h: the eleven layers in
the order mlp1, mlp2, attention, mlp3; per layer W[k][units padded to a multiple of 4], then the bias, pad entries 0) as
the master copy of the weights.  The kernel writes its .grad, a torch optimizer steps it, ebc_sarl_net_set_packed hands the
result back to the kernel's network object and SarlValueNet.refresh_from hands it to the matrix-core blocks that decide.
native=False (and every CPU device) computes the same loss and gradient with torch's autograd on SarlModule: the
comparison path, and what the CPU tests drive.  ebcsim.train.DataParallelTrainer and run_training stay what they were.

The loss is the reference's (rl/utils/trainer.py:74-100): the mean squared error between the network's value of a state and
its target.  optimize_epoch and optimize_batch are grad_train's (they take any trainer with this interface), as are the
network object's entries, the trainer around the flat tensor and the schedule's body; run_sarl_training is the schedule of
rl/train.py:99-260 on the generic pieces of ebcsim.train with this trainer in the optimizer's place and DeviceSarlPolicy
deciding.

OM-SARL (om_width = W > 0, run_sarl_training(om=spec)): mlp1's first layer takes T + W inputs, the kernel's network is
ebc_sarl_net_create_om's, the stored states are the wide ones (BatchedEnv.observe_wide_device, ebc_step_k_om) and
DeviceSarlPolicy(om=spec) decides.  The width of the maps is not in a state_dict (only T + W is): it is given explicitly.

Two forms of the kernel compute the same gradient, byte for byte (SarlNet(form=...), SarlFormTrainer(grad_form=...)): the
chunk form (ebc_sarl_net_create: one workgroup per chunk of 4 states, everything in LDS, hidden layers up to 256, R up to
what the LDS holds) and the layer form (ebc_sarl_net_create_layers: layer by layer over the batch on the float32 matrix
instruction, hidden layers up to 640, R up to 128).  Both read and write the same packed image."""
import collections
import ctypes as C
import os  # noqa: F401 (a public name of this module since its first version)

import torch

from . import _abi, grad_train
from .grad_train import (PASS_SIZES, PassChoice, _finite, checked_states_per_pass, live_states, optimize_batch,  # noqa: F401 (re-exported)
                         optimize_epoch, pad4, pick_states_per_pass)
from .sarl import DeviceSarlPolicy, SarlValueNet
from .train import SarlModule

LAYER_KEYS = ("mlp1.0", "mlp1.2", "mlp2.0", "mlp2.2", "attention.0", "attention.2", "attention.4", "mlp3.0", "mlp3.2", "mlp3.4",
              "mlp3.6")
STACKS = (("mlp1", 2), ("mlp2", 2), ("attention", 3), ("mlp3", 4))
MAX_IN, MAX_WIDTH = 64, 256  # csrc/ebc_sarl_grad_rule.h
MAX_OM, MAX_WIDE = 192, 224  # the same: the widest map behind a row, the widest row with its map
MAX_WIDTH_LAYERS, MAX_ROWS_LAYERS = 640, 128  # the same: the layer form's widest hidden layer and most rows per state
GRAD_FORMS = (None, "chunk", "layers", "auto")


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


def _views(flat, widths, self_state_dim, with_global_state):
    """An ordered dict of the reference's keys -> views into a flat packed tensor, in torch's shapes."""
    out, at = collections.OrderedDict(), 0
    for key, k, o in zip(LAYER_KEYS, layer_inputs(widths, self_state_dim, with_global_state), widths[1:]):
        at = grad_train.linear_views(out, flat, at, key, k, o)
    return out


def pack_state_dict(sd, out=None):
    """A state_dict of the reference's keys -> the packed image, flat float32 (into `out` when given)."""
    shape = shape_of(sd)
    return grad_train.pack_into(sd, out, packed_floats(*shape), sd["mlp1.0.weight"], lambda flat: _views(flat, *shape))


def unpack_to_state_dict(flat, widths, self_state_dim=6, with_global_state=True):
    """The packed image -> an ordered state_dict with SarlModule's (the reference's) keys, fresh contiguous tensors."""
    return collections.OrderedDict((k, v.clone().contiguous()) for k, v in _views(flat.detach(), widths, self_state_dim, with_global_state).items())


def module_of(sd):
    """A SarlModule of the state_dict's shape with its weights."""
    w, S, glob = shape_of(sd)
    m = SarlModule(w[0], w[1:3], w[3:5], w[8:12], w[5:8], with_global_state=glob, self_state_dim=S)
    m.load_state_dict({k: sd[k] for k in m.state_dict()})
    return m


class SarlNet(grad_train.GradNet):
    """The kernel's network object (ebc_sarl_net_*): the packed image of a state_dict in device memory."""
    KIND, ARGS = "sarl", _abi.EbcSarlGradArgs

    def __init__(self, sd, device_index, widths=None, self_state_dim=None, with_global_state=None, stack_layers=None, om_width=None,
                 form="chunk"):
        """widths / self_state_dim / with_global_state / stack_layers override what the state_dict says (the tests of the
        entry's refusals).  om_width: None = ebc_sarl_net_create; an int W = ebc_sarl_net_create_om, whose rotated width
        is mlp1.0.weight.shape[1] - W (widths[0], when given, is that rotated width).  form: "chunk" (those two entries) or
        "layers" (ebc_sarl_net_create_layers, with om_width or 0): the same packed image, hidden layers up to 640."""
        from . import _capi
        if form not in ("chunk", "layers"):
            raise ValueError("SarlNet: form is 'chunk' or 'layers', got %r" % (form,))
        self.form = form
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
        if form == "layers":
            _capi.check(self._L.ebc_sarl_net_create_layers(C.addressof(w), int(om_width or 0), int(device_index), C.byref(self._h)))
        elif om_width is None:
            _capi.check(self._L.ebc_sarl_net_create(C.addressof(w), int(device_index), C.byref(self._h)))
        else:
            _capi.check(self._L.ebc_sarl_net_create_om(C.addressof(w), int(om_width), int(device_index), C.byref(self._h)))
        self.om_width = int(om_width or 0)
        self.widths = [w.input_dim + self.om_width] + units  # [0]: the rows ebc_sarl_grad takes

    def grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, attention=None, T=None,
             states_per_pass=0):
        """One ebc_sarl_grad on the current stream: rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None,
        mask [B] uint8 or None -> grad [packed floats], loss_sum 0-d float64, count 0-d int64, value [B] float32 and
        attention [B, R] float32 when given; every tensor contiguous on the network's device.  states_per_pass: 0 = the
        whole chunk at once; 4, 2, 1 = that many of a chunk's states at a time (more rows fit, the same bytes)."""
        B, R = int(rows.shape[0]), int(rows.shape[1])
        self._grad(rows, target, grad, loss_sum, count, grad_scale, n_valid, mask, value, ("attention", attention, torch.float32, B * R), T,
                   states_per_pass)


class _NoPasses(object):
    """PassChoice's interface over a network of the layer form: every call is the default call."""

    def __init__(self, net):
        self.setting, self.whole_chunk = None, net.grad_max_rows()

    def of(self, R):
        return 0

    def max_rows(self):
        return self.whole_chunk


class SarlFormChoice(object):
    """SarlFormTrainer(grad_form="auto")'s network object: the chunk form's SarlNet where ebc_sarl_net_create(_om) takes the
    network (`chunk`, else None) and the layer form's (`layers`), made the first time a call needs it — at once when there
    is no chunk form — from current() -> (state_dict, flat packed weights on the device).  A call goes to the chunk form
    where it exists and the batch's R fits its default call, else to the layer form; set_packed reaches both."""

    def __init__(self, sd, device_index, om_width, current):
        from . import _capi
        self._index, self._om, self._current = device_index, om_width or None, current
        self.chunk = self.layers = None
        try:
            self.chunk = SarlNet(sd, device_index, om_width=self._om)
            self._chunk_rows = self.chunk.grad_max_rows()
        except _capi.EbcError as e:
            if e.code != _abi.ERR_UNSUPPORTED:
                raise
            self.layers = SarlNet(sd, device_index, om_width=self._om, form="layers")
        self.form = "chunk" if self.chunk is not None else "layers"  # of the last call (before the first: of the first network)

    def form_of(self, R):
        return "chunk" if self.chunk is not None and R <= self._chunk_rows else "layers"

    def of(self, R):
        """The network object a call on states of R rows goes to."""
        if self.form_of(R) == "chunk":
            return self.chunk
        if self.layers is None:
            sd, flat = self._current()
            self.layers = SarlNet(sd, self._index, om_width=self._om, form="layers")
            self.layers.set_packed(flat)  # the master copy's bytes themselves
        return self.layers

    def grad(self, rows, *args, **kw):
        net = self.of(int(rows.shape[1]))
        self.form = net.form
        net.grad(rows, *args, **kw)

    def packed_floats(self):
        return (self.chunk or self.layers).packed_floats()

    def grad_max_rows(self, states_per_pass=0):
        if states_per_pass:
            raise NotImplementedError("SarlFormChoice: grad_form 'auto' takes no states_per_pass")
        return MAX_ROWS_LAYERS

    def get_packed(self, out):
        return (self.chunk or self.layers).get_packed(out)

    def set_packed(self, flat):
        for net in (self.chunk, self.layers):
            if net is not None:
                net.set_packed(flat)


def checked_grad_form(value, states_per_pass, who):
    """A trainer's grad_form: None or "chunk" (the chunk form, today's object), "layers" or "auto"; the last two leave no
    room for a states_per_pass: "layers" has no passes, and "auto" is another answer to the question it answers."""
    if value not in GRAD_FORMS:
        raise ValueError("%s: grad_form is None, 'chunk', 'layers' or 'auto', got %r" % (who, value))
    if value in ("layers", "auto") and states_per_pass is not None:
        raise ValueError("%s: grad_form %r takes no states_per_pass (got %r): %s" % (
            who, value, states_per_pass, "the layer form has no passes" if value == "layers" else "they are two answers to the same question"))
    return value


class SarlTrainer(grad_train.PassTrainer):
    """module_or_state_dict: a SarlModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "sgd" (momentum 0.9), "adam" (rl/utils/trainer.py:24-45) or a callable params -> torch optimizer.  native: the kernel
    (HIP devices only; the default there) or torch autograd of SarlModule.  om_width: the W of OM-SARL's maps; the
    network's mlp1.0 then takes T + W inputs, T = widths[0] - W the rotated width (1 .. 64), W <= 192, T + W <= 224.
    states_per_pass (native only; native=False ignores it): None = the kernel's default call, the whole chunk of 4 states
    at once; 1, 2, 4 = that many states at a time, which takes more rows per state (SarlNet.grad_max_rows(S)) and gives
    the same bytes; "auto" = per call the default call where the batch's R fits it, else the largest pass that holds R.
    This trainer's kernel is the chunk form; SarlFormTrainer below adds the choice of the layer form."""

    NAME, EXTRA, OTHER_SHAPE = "SarlTrainer", "attention", "another network shape"

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None, om_width=0, states_per_pass=None):
        grad_train.PassTrainer.__init__(self, module_or_state_dict, device, optimizer, lr, native, om_width=om_width,
                                        states_per_pass=states_per_pass)

    def _configure(self, sd, om_width, states_per_pass):
        self.widths, self.self_state_dim, self.with_global_state = shape_of(sd)
        self.om_width = int(om_width)
        self.states_per_pass = checked_states_per_pass(states_per_pass, "SarlTrainer")
        if not 0 <= self.om_width <= MAX_OM:
            raise NotImplementedError("SarlTrainer: om_width %d outside 0 .. %d" % (self.om_width, MAX_OM))
        if self.widths[0] - self.om_width < 1:
            raise ValueError("SarlTrainer: om_width %d leaves no rotated columns of mlp1.0's %d inputs" % (self.om_width, self.widths[0]))
        if self.om_width and self.widths[0] > MAX_WIDE:
            raise NotImplementedError("SarlTrainer: T + om_width = %d columns, the gradient takes up to %d" % (self.widths[0], MAX_WIDE))

    _shape_of, _pack, _module_of = staticmethod(shape_of), staticmethod(pack_state_dict), staticmethod(module_of)
    _param_key = staticmethod(SarlModule._ref_name)

    def _shape(self):
        return self.widths, self.self_state_dim, self.with_global_state

    def _views(self, flat):
        return _views(flat, *self._shape())

    def _new_pass_net(self, sd, index):
        return SarlNet(sd, index, om_width=self.om_width or None)

    def loss_and_grad(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, attention=None):
        """rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None, mask [B] uint8 / bool or None, on the
        trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64) there; .grad of the master copy holds
        d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 2 / count, torch's MSELoss over the live states (this
        reads the count back).  value [B] float32 / attention [B, R] float32, when given, receive the states' values and
        softmax weights (native only)."""
        return self._loss_and_grad(rows, target, n_valid, mask, grad_scale, value, attention)


class SarlFormTrainer(SarlTrainer):
    """SarlTrainer with the choice of the kernel's form: its arguments, and grad_form (native only; native=False ignores
    it): None or "chunk" = SarlTrainer's object, the chunk form, refusals included; "layers" = the layer form (hidden layers
    up to 640, R up to 128; states_per_pass must be None); "auto" = per call the chunk form where ebc_sarl_net_create(_om)
    takes the network and the batch's R fits its default call, else the layer form, whose network object is made the first
    time it is needed and follows push_weights.  The rule is about capability, not speed: the bytes are the same on both
    forms.  "auto" with a states_per_pass is a ValueError.  (A class of its own: SarlTrainer's constructor keeps its
    signature.)"""

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None, om_width=0, states_per_pass=None,
                 grad_form=None):
        self.grad_form = checked_grad_form(grad_form, states_per_pass, "SarlFormTrainer")
        SarlTrainer.__init__(self, module_or_state_dict, device, optimizer, lr, native, om_width, states_per_pass)

    def _new_net(self, sd, index):
        """None / "chunk": PassTrainer's network object.  "layers": the layer form's.  "auto": both forms behind one object
        (SarlFormChoice), which routes every call by its R."""
        if self.grad_form in (None, "chunk"):
            return grad_train.PassTrainer._new_net(self, sd, index)
        if self.grad_form == "layers":
            net = SarlNet(sd, index, om_width=self.om_width or None, form="layers")
        else:
            net = SarlFormChoice(sd, index, self.om_width, lambda: (self.state_dict(), self.flat.detach()))
        self.passes = _NoPasses(net)
        return net

    def form_of(self, R):
        """"chunk" or "layers": the form a native call on states of R rows takes."""
        if self.grad_form == "auto":
            return self.net.form_of(R) if self.net is not None else ("chunk" if max(self.widths[1:]) <= MAX_WIDTH else "layers")
        return "layers" if self.grad_form == "layers" else "chunk"


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
    Returns a dict of what happened.  (run_sarl_training_ex below: the same with the choice of the deciding blocks.)"""
    return run_sarl_training_ex(env, trainer, actions, gamma, il_steps=il_steps, il_epochs=il_epochs, il_learning_rate=il_learning_rate,
                                il_safety_space=il_safety_space, rl_learning_rate=rl_learning_rate, train_iterations=train_iterations,
                                steps_per_iteration=steps_per_iteration, train_batches=train_batches, batch_size=batch_size,
                                capacity=capacity, epsilon_start=epsilon_start, epsilon_end=epsilon_end, epsilon_decay=epsilon_decay,
                                target_update_interval=target_update_interval, generator=generator, log=log, output_dir=output_dir,
                                checkpoint_interval=checkpoint_interval, rank=rank, after_il=after_il, om=om)


def run_sarl_training_ex(env, trainer, actions, gamma, wide_decide=False, il_steps=0, il_epochs=0, il_learning_rate=0.01, il_safety_space=0.15,
                         rl_learning_rate=0.001, train_iterations=0, steps_per_iteration=1, train_batches=100, batch_size=100,
                         capacity=100000, epsilon_start=0.5, epsilon_end=0.1, epsilon_decay=4000, target_update_interval=50,
                         generator=None, log=None, output_dir=None, checkpoint_interval=0, rank=0, after_il=None, om=None):
    """run_sarl_training (its arguments, its checks, its result) with one keyword more.  wide_decide: the deciding and
    the target network take wide blocks for the stacks the narrow block does not hold (SarlValueNet(..., wide=True): the
    networks the layer form of the gradient trains); False: such networks decide on torch, which is run_sarl_training.
    (A function of its own: run_sarl_training keeps its signature.)"""
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
    om_kw = {} if om is None else {"om": om}  # without maps: the calls as they were
    kw = dict(device=dev, with_global_state=trainer.with_global_state, self_state_dim=trainer.self_state_dim)
    if wide_decide:
        kw["wide"] = True
    return grad_train.run_value_training(
        env, trainer, gamma, env.T + W, lambda: SarlValueNet(trainer.state_dict(), **kw), lambda net: DeviceSarlPolicy(net, actions, gamma, **om_kw),
        lambda net: net.refresh_from(trainer), om_kw, om_kw, il_steps, il_epochs, il_learning_rate, il_safety_space, rl_learning_rate,
        train_iterations, steps_per_iteration, train_batches, batch_size, capacity, epsilon_start, epsilon_end, epsilon_decay,
        target_update_interval, generator, log, output_dir, checkpoint_interval, rank, after_il)
