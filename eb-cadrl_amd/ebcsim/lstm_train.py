"""Training the LSTM-RL value networks on the device: rollouts -> the fused forward + backward-through-time kernel
(ebc_lstm_grad, csrc/ebc_lstm_grad.h) -> a torch optimizer -> a state_dict in the reference's ValueNetwork1 / ValueNetwork2
layout (mlp1.*, lstm.weight_ih_l0 ..., mlp.*; rl/policy/lstm_rl.py:9-69) that tools/evaluate.py --policy lstm_rl loads.

LstmTrainer keeps ONE flat float32 tensor in the kernel's packed layout (csrc/ebc_lstm_grad_rule.h: mlp1's layers, then
w_ih[k][4 H], w_hh[k][4 H], b_ih, b_hh, then mlp's layers; a Linear layer as W[k][units padded to a multiple of 4], then the
bias, pad entries 0) as the master copy of the weights.  b_ih and b_hh are both there and receive the same gradient, so a
torch optimizer stepping the flat tensor moves the weights exactly as it would move LstmModule's parameters.  The kernel
writes its .grad, the optimizer steps it, ebc_lstm_net_set_packed hands the result back to the kernel's network object and
LstmValueNet.refresh_from hands it to the blocks and the scan that decide.  native=False (and every CPU device) computes
the same loss and gradient with torch's autograd on LstmModule: the comparison path, and what the CPU tests drive.

The loss is the reference's (rl/utils/trainer.py:74-100).  optimize_epoch and optimize_batch are grad_train's, as are the
network object's entries, the trainer around the flat tensor and the schedule's body; run_lstm_training is the schedule of
rl/train.py:99-260 with this trainer in the optimizer's place and DeviceSarlPolicy over LstmValueNet deciding.  It differs
from run_sarl_training in what the reference itself does differently: in RL mode the replay holds the policy's last_state,
whose rows LstmRL.predict has sorted by decreasing distance to the robot (lstm_rl.py:117-123, explorer.py:44), and the next
state the target network values is sorted the same way; the imitation states stay in the env's order (explorer.py:161).

OM-LSTM ([lstm_rl] with_om = true) is the same trainer and schedule on rows T + W wide (13 + 4 * 4 * 3 = 61 at the
reference's settings; the kernels take up to 64): run_lstm_training(..., om=spec) fills the replay with wide states — the
imitation window's from ebc_step_k_om in the env's order, the RL rounds' from ebc_observe_wide_sorted, whose maps are built
from the rows in the sorted order as the reference's transform(state) builds them — and DeviceSarlPolicy(om=spec) decides."""
import collections
import ctypes as C
import os  # noqa: F401 (a public name of this module since its first version)

import torch

from . import _abi, grad_train
from .grad_train import (PASS_SIZES, PassChoice, _finite, checked_states_per_pass, live_states, optimize_batch,  # noqa: F401 (re-exported)
                         optimize_epoch, pad4, pick_states_per_pass)
from .lstm_rl import LstmModule, LstmValueNet
from .sarl import DeviceSarlPolicy

MLP1_KEYS = ("mlp1.0", "mlp1.2", "mlp1.4", "mlp1.6")
MLP_KEYS = ("mlp.0", "mlp.2", "mlp.4", "mlp.6")
LSTM_KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0")
MAX_IN, MAX_WIDTH, MAX_DIM = 64, 256, 64  # csrc/ebc_lstm_grad_rule.h, csrc/ebc_lstm_cell.h
DISTANCE_COLUMN = 11  # `da` of a rotated row (multi_human_rl.py:128-149): the distance between the robot and the row's agent


def _linear_keys(sd, prefix):
    return ["%s.%d" % (prefix, i) for i in sorted({int(k.split(".")[1]) for k in sd if k.startswith(prefix + ".") and k.endswith(".weight")})]


def shape_of(sd):
    """(widths, self_state_dim, with_interaction_module) of a state_dict with the reference's keys; widths = [row width,
    mlp1's four units (zeros without mlp1), H, mlp's four units]."""
    k1, k = _linear_keys(sd, "mlp1"), _linear_keys(sd, "mlp")
    if (k1 and k1 != list(MLP1_KEYS)) or k != list(MLP_KEYS) or any(key not in sd for key in LSTM_KEYS):
        raise NotImplementedError("LSTM-RL training: mlp1 of 0 or 4 Linear layers, mlp of 4 (%s) and one LSTM layer, got %s / %s"
                                  % (", ".join(MLP_KEYS), k1, k))
    two = bool(k1)
    H = int(sd["lstm.weight_hh_l0"].shape[1])
    I = int(sd["lstm.weight_ih_l0"].shape[1])
    T = int(sd["mlp1.0.weight"].shape[1]) if two else I
    m1 = [int(sd[key + ".weight"].shape[0]) for key in MLP1_KEYS] if two else [0, 0, 0, 0]
    if two and m1[-1] != I:
        raise ValueError("the LSTM takes %d inputs, mlp1 gives %d" % (I, m1[-1]))
    return [T] + m1 + [H] + [int(sd[key + ".weight"].shape[0]) for key in MLP_KEYS], int(sd["mlp.0.weight"].shape[1]) - H, two


def _layout(widths, self_state_dim, two):
    """[(key, kind, inputs, units)] in the packed order; kind "linear" (W[k][Op] | bias[Op]) or "cell"."""
    T, H = widths[0], widths[5]
    out, k = [], T
    if two:
        for key, o in zip(MLP1_KEYS, widths[1:5]):
            out.append((key, "linear", k, o))
            k = o
    out.append(("lstm", "cell", k, H))
    k = int(self_state_dim) + H
    for key, o in zip(MLP_KEYS, widths[6:10]):
        out.append((key, "linear", k, o))
        k = o
    return out


def packed_floats(widths, self_state_dim=6, two=True):
    return sum((k + 1) * pad4(o) if kind == "linear" else (k + o + 2) * 4 * o for _, kind, k, o in _layout(widths, self_state_dim, two))


def _views(flat, widths, self_state_dim, two):
    """An ordered dict of the reference's keys -> views into a flat packed tensor, in torch's shapes."""
    out, at = collections.OrderedDict(), 0
    for key, kind, k, o in _layout(widths, self_state_dim, two):
        if kind == "linear":
            at = grad_train.linear_views(out, flat, at, key, k, o)
        else:
            h4 = 4 * o
            out[LSTM_KEYS[0]] = flat[at:at + k * h4].view(k, h4).t()
            out[LSTM_KEYS[1]] = flat[at + k * h4:at + (k + o) * h4].view(o, h4).t()
            out[LSTM_KEYS[2]] = flat[at + (k + o) * h4:at + (k + o + 1) * h4]
            out[LSTM_KEYS[3]] = flat[at + (k + o + 1) * h4:at + (k + o + 2) * h4]
            at += (k + o + 2) * h4
    return out


def pack_state_dict(sd, out=None):
    """A state_dict of the reference's keys -> the packed image, flat float32 (into `out` when given)."""
    shape = shape_of(sd)
    return grad_train.pack_into(sd, out, packed_floats(*shape), sd["mlp.0.weight"], lambda flat: _views(flat, *shape))


def unpack_to_state_dict(flat, widths, self_state_dim=6, two=True):
    """The packed image -> an ordered state_dict with LstmModule's (the reference's) keys, fresh contiguous tensors."""
    return collections.OrderedDict((k, v.clone().contiguous()) for k, v in _views(flat.detach(), widths, self_state_dim, two).items())


def module_of(sd):
    """An LstmModule of the state_dict's shape with its weights."""
    _, S, _ = shape_of(sd)
    return LstmModule.from_state_dict({k: v.detach() for k, v in sd.items()}, S)


def distance_order(rows, n_valid=None):
    """LstmRL.predict's order (lstm_rl.py:117-123: sorted by the distance to the robot, reverse=True) of rotated rows, on
    their device: for each state the indices of its existing rows [0, n_valid) in a stable descending order of their own
    distance column (index 11, `da`), then the padding rows where they are, at the end.  rows [B, R, >= 12] -> int64 [B, R];
    n_valid [B] or None = all R."""
    R = rows.shape[1]
    key = -rows[:, :, DISTANCE_COLUMN]
    last = torch.full_like(key, float("inf"))
    key = torch.where(key != key, last, key)  # a NaN distance sorts behind every number, as +inf does: a stable sort then
    if n_valid is not None:                   # keeps the padding rows (+inf too, at the higher indices) behind every row
        key = torch.where(torch.arange(R, device=rows.device)[None, :] < n_valid.to(rows.device)[:, None], key, last)
    return torch.sort(key, dim=1, stable=True).indices


def sort_rows_by_distance(rows, n_valid=None):
    """The rows of each state in distance_order: rows [B, R, T]; n_valid [B] or None = all R."""
    order = distance_order(rows, n_valid)
    return torch.gather(rows, 1, order[:, :, None].expand_as(rows))


class LstmNet(grad_train.GradNet):
    """The kernel's network object (ebc_lstm_net_*): the packed image of a state_dict in device memory."""
    KIND, ARGS = "lstm", _abi.EbcLstmGradArgs

    def __init__(self, sd, device_index):
        from . import _capi
        self._L = _capi.lib()
        widths, S, two = shape_of(sd)
        host = {k: v.detach().to("cpu", torch.float32).contiguous().numpy() for k, v in sd.items()}
        self._keep = host
        w = _abi.EbcLstmNetWeights()
        w.struct_size = C.sizeof(w)
        w.n_mlp1, w.n_mlp = (4 if two else 0), 4
        w.self_state_dim = S
        w.input_dim, w.hidden_dim, w.lstm_input_dim = widths[0], widths[5], int(sd[LSTM_KEYS[0]].shape[1])
        for i, key in enumerate(MLP1_KEYS if two else ()):
            w.widths[i], w.weight[i], w.bias[i] = widths[1 + i], host[key + ".weight"].ctypes.data, host[key + ".bias"].ctypes.data
        for i, key in enumerate(MLP_KEYS):
            w.widths[4 + i], w.weight[4 + i], w.bias[4 + i] = widths[6 + i], host[key + ".weight"].ctypes.data, host[key + ".bias"].ctypes.data
        w.w_ih, w.w_hh, w.b_ih, w.b_hh = (host[k].ctypes.data for k in LSTM_KEYS)
        self._h = C.c_void_p()
        _capi.check(self._L.ebc_lstm_net_create(C.addressof(w), int(device_index), C.byref(self._h)))
        self.widths, self.self_state_dim, self.two = widths, S, two
        self.joint_dim = S + widths[5]

    def grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, joint=None, T=None,
             states_per_pass=0):
        """One ebc_lstm_grad on the current stream: rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None,
        mask [B] uint8 or None -> grad [packed floats], loss_sum 0-d float64, count 0-d int64, value [B] float32 and
        joint [B, S + H] float32 when given; every tensor contiguous on the network's device.  states_per_pass: 0 = the
        whole chunk at once; 4, 2, 1 = that many of a chunk's states at a time (more rows fit, the same bytes)."""
        self._grad(rows, target, grad, loss_sum, count, grad_scale, n_valid, mask, value,
                   ("joint", joint, torch.float32, int(rows.shape[0]) * self.joint_dim), T, states_per_pass)


class LstmTrainer(grad_train.PassTrainer):
    """module_or_state_dict: an LstmModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "sgd" (momentum 0.9), "adam" (rl/utils/trainer.py:24-45) or a callable params -> torch optimizer.  native: the kernel
    (HIP devices only; the default there) or torch autograd of LstmModule.  states_per_pass (native only; native=False
    ignores it): None = the kernel's default call, the whole chunk of 4 states at once; 1, 2, 4 = that many states at a
    time, which takes more rows per state (LstmNet.grad_max_rows(S)) and gives the same bytes; "auto" = per call the
    default call where the batch's R fits it, else the largest pass that holds R."""

    NAME, EXTRA, OTHER_SHAPE = "LstmTrainer", "joint", "another network shape"

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None, states_per_pass=None):
        grad_train.PassTrainer.__init__(self, module_or_state_dict, device, optimizer, lr, native, states_per_pass=states_per_pass)

    def _configure(self, sd, states_per_pass):
        self.widths, self.self_state_dim, self.with_interaction_module = shape_of(sd)
        self.states_per_pass = checked_states_per_pass(states_per_pass, "LstmTrainer")

    _shape_of, _pack, _module_of, _new_pass_net = staticmethod(shape_of), staticmethod(pack_state_dict), staticmethod(module_of), LstmNet

    def _shape(self):
        return self.widths, self.self_state_dim, self.with_interaction_module

    def _views(self, flat):
        return _views(flat, *self._shape())

    def _forward(self, x, n_valid):
        return self.module(x, n_valid).squeeze(1)

    def loss_and_grad(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, joint=None):
        """rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None, mask [B] uint8 / bool or None, on the
        trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64) there; .grad of the master copy holds
        d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 2 / count, torch's MSELoss over the live states (this
        reads the count back).  value [B] float32 / joint [B, S + H] float32, when given, receive the states' values and
        mlp's inputs (native only)."""
        return self._loss_and_grad(rows, target, n_valid, mask, grad_scale, value, joint)


def run_lstm_training(env, trainer, actions, gamma, il_steps=0, il_epochs=0, il_learning_rate=0.01, il_safety_space=0.15,
                      rl_learning_rate=0.001, train_iterations=0, steps_per_iteration=1, train_batches=100, batch_size=100,
                      capacity=100000, epsilon_start=0.5, epsilon_end=0.1, epsilon_decay=4000, target_update_interval=50,
                      generator=None, log=None, output_dir=None, checkpoint_interval=0, rank=0, after_il=None, om=None):
    """The schedule of sarl_train.run_sarl_training (rl/train.py:99-260) for LSTM-RL on one rank's env slice: imitation
    learning with the robot on ORCA (its states in the env's order, explorer.py:161), then `train_iterations` rounds of
    [epsilon-greedy rollout with DeviceSarlPolicy over LstmValueNet, the stored state and the next state the target network
    values sorted by sort_rows_by_distance (lstm_rl.py:117-123, explorer.py:44) -> `train_batches` optimizer steps on
    DeviceReplay samples -> the deciding network's tensors, blocks and scan refreshed from the trainer on the device], the
    target network refreshed every `target_update_interval` rounds.  env: BatchedEnv with auto-reset semantics (a scene
    pool) on the trainer's HIP device, rows 13 wide.  output_dir: `il_model.pth` after imitation learning and
    `rl_model_<round>.pth` every `checkpoint_interval` rounds and at the end.  A reward, value target or loss that is not
    finite raises FloatingPointError at once, before an optimizer step sees it.  Returns a dict of what happened.
    om (an occupancy.OccupancySpec): OM-LSTM.  The network's rows are env.T + om.width wide; the imitation states are
    collect_il(om=om)'s (the env's order with maps), the RL rounds' stored and next states are
    collect(om=om, sorted_rows=True)'s (one observe_wide_sorted_device after the step is both) and DeviceSarlPolicy(om=om)
    decides.  None changes no byte and no launch."""
    dev = trainer.device
    if dev.type != "cuda":
        raise NotImplementedError("run_lstm_training: the rollouts run on a HIP device")
    width = env.T + (om.width if om is not None else 0)
    if width != trainer.widths[0]:
        if om is not None:
            raise NotImplementedError("run_lstm_training: the env's rows are %d wide and the maps add %d, the network takes %d"
                                      % (env.T, om.width, trainer.widths[0]))
        raise NotImplementedError("run_lstm_training: the env's rows are %d wide, the network takes %d (LSTM-RL runs with "
                                  "with_agent_type = 0; OM-LSTM needs om=)" % (env.T, trainer.widths[0]))
    if trainer.native and env.R > trainer.grad_max_rows():
        raise NotImplementedError("run_lstm_training: %d rows per state, ebc_lstm_grad takes %d for this network; use native=False"
                                  % (env.R, trainer.grad_max_rows()))
    # without maps the calls stay as they were: the RL rounds' states sorted here; with them the env sorts and maps (sorted_rows)
    om_kw = {} if om is None else {"om": om}
    collect_kw = {"state_transform": sort_rows_by_distance} if om is None else {"om": om, "sorted_rows": True}
    return grad_train.run_value_training(
        env, trainer, gamma, width, lambda: LstmValueNet(trainer.state_dict(), device=dev, self_state_dim=trainer.self_state_dim),
        lambda net: DeviceSarlPolicy(net, actions, gamma, **om_kw), lambda net: net.refresh_from(trainer), om_kw, collect_kw, il_steps,
        il_epochs, il_learning_rate, il_safety_space, rl_learning_rate, train_iterations, steps_per_iteration, train_batches, batch_size,
        capacity, epsilon_start, epsilon_end, epsilon_decay, target_update_interval, generator, log, output_dir, checkpoint_interval, rank,
        after_il)
