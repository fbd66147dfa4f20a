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
EpisodeStore, DeviceReplay) with this trainer in the optimizer's place.  What CADRL shares with SARL and LSTM-RL (the
network object's entries, the trainer around the flat tensor, the optimizer loops, the schedule) is grad_train's."""
import collections
import ctypes as C
import os  # noqa: F401 (a public name of this module since its first version)

import torch

from . import _abi, grad_train
from .cadrl import CadrlModule, CadrlValueNet, DeviceCadrlPolicy
from .grad_train import _finite, live_states, optimize_batch, optimize_epoch, pad4  # noqa: F401 (re-exported)

LAYER_KEYS = ("value_network.0", "value_network.2", "value_network.4", "value_network.6")
MAX_IN, MAX_WIDTH, MAX_ROWS = 64, 256, 128  # csrc/ebc_cadrl_grad_rule.h, csrc/ebc_cadrl_rule.h


def widths_of(sd):
    """[row width, units of layer 1 .. 4] of a state_dict with the reference's keys."""
    keys = sorted(k for k in sd if k.startswith("value_network.") and k.endswith(".weight"))
    if [k[:-len(".weight")] for k in keys] != list(LAYER_KEYS):
        raise NotImplementedError("CADRL training: value_network is four Linear layers (value_network.0, .2, .4, .6), got %s" % keys)
    return [int(sd[LAYER_KEYS[0] + ".weight"].shape[1])] + [int(sd[k + ".weight"].shape[0]) for k in LAYER_KEYS]


def packed_floats(widths):
    return sum((k + 1) * pad4(o) for k, o in zip(widths[:-1], widths[1:]))


def _views(flat, widths):
    """An ordered dict of the reference's keys -> views into a flat packed tensor, in torch's shapes."""
    out, at = collections.OrderedDict(), 0
    for key, k, o in zip(LAYER_KEYS, widths[:-1], widths[1:]):
        at = grad_train.linear_views(out, flat, at, key, k, o)
    return out


def pack_state_dict(sd, out=None):
    """A state_dict of the reference's keys -> the packed image, flat float32 (into `out` when given)."""
    widths = widths_of(sd)
    return grad_train.pack_into(sd, out, packed_floats(widths), sd[LAYER_KEYS[0] + ".weight"], lambda flat: _views(flat, widths))


def unpack_to_state_dict(flat, widths):
    """The packed image -> an ordered state_dict with CadrlModule's (the reference's) keys, fresh contiguous tensors."""
    return collections.OrderedDict((k, v.clone().contiguous()) for k, v in _views(flat.detach(), widths).items())


class CadrlNet(grad_train.GradNet):
    """The kernel's network object (ebc_cadrl_net_*): the packed image of a state_dict in device memory."""
    KIND, ARGS = "cadrl", _abi.EbcCadrlGradArgs

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

    def grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, min_row=None):
        """One ebc_cadrl_grad on the current stream: rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None,
        mask [B] uint8 or None -> grad [packed floats], loss_sum 0-d float64, count 0-d int64, value [B] float32 and
        min_row [B] int32 when given; every tensor contiguous on the network's device."""
        self._grad(rows, target, grad, loss_sum, count, grad_scale, n_valid, mask, value, ("min_row", min_row, torch.int32, int(rows.shape[0])))


class CadrlTrainer(grad_train.GradTrainer):
    """module_or_state_dict: a CadrlModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "sgd" (momentum 0.9), "adam" (rl/utils/trainer.py:24-45) or a callable params -> torch optimizer.  native: the kernel
    (HIP devices only; the default there) or torch autograd of CadrlModule."""
    NAME, EXTRA, OTHER_SHAPE = "CadrlTrainer", "min_row", "other layer widths"

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None):
        grad_train.GradTrainer.__init__(self, module_or_state_dict, device, optimizer, lr, native)

    def _configure(self, sd):
        self.widths = widths_of(sd)

    _shape_of, _pack = staticmethod(widths_of), staticmethod(pack_state_dict)
    _module_of, _new_net = CadrlModule.from_state_dict, CadrlNet

    def _shape(self):
        return self.widths

    def _views(self, flat):
        return _views(flat, self.widths)

    def loss_and_grad(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, min_row=None):
        """rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None, mask [B] uint8 / bool or None, on the
        trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64) there; .grad of the master copy holds
        d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 2 / count, torch's MSELoss over the live states (this
        reads the count back).  value [B] float32 / min_row [B] int32, when given, receive the states' values and the
        rows they came from (native only)."""
        return self._loss_and_grad(rows, target, n_valid, mask, grad_scale, value, min_row)


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
    dev = trainer.device
    if dev.type != "cuda":
        raise NotImplementedError("run_cadrl_training: the rollouts run on a HIP device")
    return grad_train.run_value_training(
        env, trainer, gamma, env.T, lambda: CadrlValueNet(trainer.state_dict(), device=dev), lambda net: DeviceCadrlPolicy(net, actions, gamma),
        lambda net: net.refresh_native(trainer), {}, {}, il_steps, il_epochs, il_learning_rate, il_safety_space, rl_learning_rate,
        train_iterations, steps_per_iteration, train_batches, batch_size, capacity, epsilon_start, epsilon_end, epsilon_decay,
        target_update_interval, generator, log, output_dir, checkpoint_interval, rank, after_il)
