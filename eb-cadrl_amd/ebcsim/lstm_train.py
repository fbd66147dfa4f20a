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

The loss is the reference's (rl/utils/trainer.py:74-100).  optimize_epoch and optimize_batch are cadrl_train's;
run_lstm_training is the schedule of rl/train.py:99-260 with this trainer in the optimizer's place and DeviceSarlPolicy
over LstmValueNet deciding.  It differs from run_sarl_training in what the reference itself does differently: in RL mode
the replay holds the policy's last_state, whose rows LstmRL.predict has sorted by decreasing distance to the robot
(lstm_rl.py:117-123, explorer.py:44), and the next state the target network values is sorted the same way; the imitation
states stay in the env's order (explorer.py:161).

OM-LSTM ([lstm_rl] with_om = true) is the same trainer and schedule on rows T + W wide (13 + 4 * 4 * 3 = 61 at the
reference's settings; the kernels take up to 64): run_lstm_training(..., om=spec) fills the replay with wide states — the
imitation window's from ebc_step_k_om in the env's order, the RL rounds' from ebc_observe_wide_sorted, whose maps are built
from the rows in the sorted order as the reference's transform(state) builds them — and DeviceSarlPolicy(om=spec) decides."""
import collections
import ctypes as C
import os

import torch

from . import _abi
from .cadrl_train import _finite, live_states, optimize_batch, optimize_epoch, pad4  # noqa: F401 (re-exported)
from .lstm_rl import LstmModule, LstmValueNet
from .sarl import DeviceSarlPolicy
from .sarl_train import PASS_SIZES, PassChoice, checked_states_per_pass, pick_states_per_pass  # noqa: F401 (re-exported)

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
            op = pad4(o)
            out[key + ".weight"] = flat[at:at + k * op].view(k, op)[:, :o].t()
            out[key + ".bias"] = flat[at + k * op:at + (k + 1) * op][:o]
            at += (k + 1) * op
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
    widths, S, two = shape_of(sd)
    if out is None:
        out = torch.zeros(packed_floats(widths, S, two), dtype=torch.float32, device=sd["mlp.0.weight"].device)
    else:
        out.zero_()
    with torch.no_grad():
        for key, v in _views(out, widths, S, two).items():
            v.copy_(sd[key])
    return out


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


class LstmNet(object):
    """The kernel's network object (ebc_lstm_net_*): the packed image of a state_dict in device memory."""

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

    def packed_floats(self):
        from . import _capi
        n = C.c_int64()
        _capi.check(self._L.ebc_lstm_net_packed_floats(self._h, C.byref(n)))
        return int(n.value)

    def grad_max_rows(self, states_per_pass=0):
        """The largest R ebc_lstm_grad takes for this network: a chunk's activations (states_per_pass 4, 2, 1: those of
        that many states) fit a workgroup's LDS."""
        from . import _capi
        n = C.c_int()
        if states_per_pass == 0:
            _capi.check(self._L.ebc_lstm_net_grad_max_rows(self._h, C.byref(n)))
        else:
            _capi.check(self._L.ebc_lstm_net_grad_max_rows_at(self._h, int(states_per_pass), C.byref(n)))
        return int(n.value)

    def get_packed(self, out):
        from . import _capi
        assert out.dtype == torch.float32 and out.is_contiguous() and out.is_cuda and out.numel() == self.packed_floats()
        _capi.check(self._L.ebc_lstm_net_get_packed(self._h, torch.cuda.current_stream(out.device).cuda_stream, out.data_ptr()))
        return out

    def set_packed(self, flat):
        from . import _capi
        assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.is_cuda and flat.numel() == self.packed_floats()
        _capi.check(self._L.ebc_lstm_net_set_packed(self._h, torch.cuda.current_stream(flat.device).cuda_stream, flat.data_ptr()))

    def grad(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, joint=None, T=None,
             states_per_pass=0):
        """One ebc_lstm_grad on the current stream: rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None,
        mask [B] uint8 or None -> grad [packed floats], loss_sum 0-d float64, count 0-d int64, value [B] float32 and
        joint [B, S + H] float32 when given; every tensor contiguous on the network's device.  states_per_pass: 0 = the
        whole chunk at once; 4, 2, 1 = that many of a chunk's states at a time (more rows fit, the same bytes)."""
        from . import _capi
        B, R, Tr = (int(x) for x in rows.shape)
        a = _abi.EbcLstmGradArgs()
        a.struct_size = C.sizeof(a)
        a.B, a.R, a.T, a.grad_scale = B, R, Tr if T is None else int(T), float(grad_scale)
        a.states_per_pass = int(states_per_pass)
        for name, t, dtype, numel in (("rows", rows, torch.float32, B * R * Tr), ("target", target, torch.float32, B),
                                      ("n_valid", n_valid, torch.int64, B), ("sample_mask", mask, torch.uint8, B),
                                      ("grad", grad, torch.float32, self.packed_floats()), ("loss_sum", loss_sum, torch.float64, 1),
                                      ("count", count, torch.int64, 1), ("value", value, torch.float32, B),
                                      ("joint", joint, torch.float32, B * self.joint_dim)):
            if t is None:
                continue
            assert t.dtype == dtype and t.is_contiguous() and t.is_cuda and t.numel() == numel, name
            setattr(a, name, t.data_ptr())
        _capi.check(self._L.ebc_lstm_grad(self._h, torch.cuda.current_stream(rows.device).cuda_stream, C.addressof(a)))

    def __del__(self):
        try:
            self._L.ebc_lstm_net_destroy(self._h)
        except Exception:
            pass


class LstmTrainer(object):
    """module_or_state_dict: an LstmModule or a state_dict of the reference's keys (the starting weights).  optimizer:
    "sgd" (momentum 0.9), "adam" (rl/utils/trainer.py:24-45) or a callable params -> torch optimizer.  native: the kernel
    (HIP devices only; the default there) or torch autograd of LstmModule.  states_per_pass (native only; native=False
    ignores it): None = the kernel's default call, the whole chunk of 4 states at once; 1, 2, 4 = that many states at a
    time, which takes more rows per state (LstmNet.grad_max_rows(S)) and gives the same bytes; "auto" = per call the
    default call where the batch's R fits it, else the largest pass that holds R."""

    def __init__(self, module_or_state_dict, device="cpu", optimizer="sgd", lr=0.01, native=None, states_per_pass=None):
        sd = module_or_state_dict.state_dict() if isinstance(module_or_state_dict, torch.nn.Module) else module_or_state_dict
        sd = collections.OrderedDict((k, v.detach().to("cpu", torch.float32)) for k, v in sd.items())
        self.device = torch.device(device)
        self.widths, self.self_state_dim, self.with_interaction_module = shape_of(sd)
        self.states_per_pass = checked_states_per_pass(states_per_pass, "LstmTrainer")
        self.native = (self.device.type == "cuda") if native is None else bool(native)
        if self.native and self.device.type != "cuda":
            raise NotImplementedError("LstmTrainer(native=True) needs a HIP device: the kernel has no CPU form")
        self.flat = pack_state_dict(sd).to(self.device).requires_grad_(True)
        self.flat.grad = torch.zeros_like(self.flat)
        self._optimizer_spec = optimizer
        self.set_learning_rate(lr)
        self.module = module_of(sd).to(self.device)  # the autograd path's
        self.net = None
        if self.native:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.net = LstmNet(sd, idx)
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
        return _views(flat, self.widths, self.self_state_dim, self.with_interaction_module)

    # ------------------------------------------------------------------ weights
    def state_dict(self):
        return unpack_to_state_dict(self.flat.detach().cpu(), self.widths, self.self_state_dim, self.with_interaction_module)

    def device_state_dict(self):
        """The reference's keys as views into the master copy on its device (no copy): what LstmValueNet.refresh_from reads."""
        return self._views(self.flat.detach())

    def save(self, path):
        """The current weights as a file torch.save wrote: loads into LstmModule and the reference's ValueNetwork1 /
        ValueNetwork2 with strict=True."""
        torch.save(self.state_dict(), path)

    def load_state_dict(self, sd):
        if shape_of(sd) != (self.widths, self.self_state_dim, self.with_interaction_module):
            raise ValueError("LstmTrainer.load_state_dict: another network shape")
        with torch.no_grad():
            pack_state_dict({k: v.to(self.device, torch.float32) for k, v in sd.items()}, out=self.flat)
        self.push_weights()

    def push_weights(self):
        """The master copy into the kernel's network object (ebc_lstm_net_set_packed on the current stream)."""
        if self.net is not None:
            self.net.set_packed(self.flat.detach())

    def _load_module(self):
        with torch.no_grad():
            params = dict(self.module.named_parameters())
            for key, v in self._views(self.flat.detach()).items():
                params[key].copy_(v)

    # ------------------------------------------------------------------ loss and gradient
    def loss_and_grad(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, joint=None):
        """rows [B, R, T] float32, target [B] float32, n_valid [B] int64 or None, mask [B] uint8 / bool or None, on the
        trainer's device -> (loss_sum, count) as 0-d tensors (float64, int64) there; .grad of the master copy holds
        d/dweights of grad_scale / 2 * loss_sum.  grad_scale None: 2 / count, torch's MSELoss over the live states (this
        reads the count back).  value [B] float32 / joint [B, S + H] float32, when given, receive the states' values and
        mlp's inputs (native only)."""
        rows, target = rows.to(self.device, torch.float32).contiguous(), target.to(self.device, torch.float32).reshape(-1).contiguous()
        B, R, T = (int(x) for x in rows.shape)
        if T != self.widths[0]:
            raise ValueError("LstmTrainer: rows are %d wide, the network takes %d" % (T, self.widths[0]))
        live = None
        if grad_scale is None:
            live = live_states(B, R, n_valid, mask, self.device)
            grad_scale = 2.0 / max(int(live.sum()), 1)
        if self.native:
            loss = torch.empty((), dtype=torch.float64, device=self.device)
            count = torch.empty((), dtype=torch.int64, device=self.device)
            nv = None if n_valid is None else n_valid.to(device=self.device, dtype=torch.int64).contiguous()
            mk = None if mask is None else mask.to(device=self.device).to(torch.uint8).contiguous()
            self.net.grad(rows, target, self.flat.grad, loss, count, grad_scale, nv, mk, value, joint, states_per_pass=self.passes.of(R))
            return loss, count
        if value is not None or joint is not None:
            raise NotImplementedError("LstmTrainer(native=False): `value` and `joint` are the kernel's outputs")
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
            out = self.module(x, nv).squeeze(1)
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
    import torch.distributed as dist
    from .train import DeviceReplay, EpisodeStore, _multi_rank, all_ranks, collect, collect_il
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
        if om is None:
            hist["il_stored"], hist["il_episodes"] = collect_il(env, memory, il_steps, gamma, il_safety_space)
        else:
            hist["il_stored"], hist["il_episodes"] = collect_il(env, memory, il_steps, gamma, il_safety_space, om=om)
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
    net = LstmValueNet(trainer.state_dict(), device=dev, self_state_dim=trainer.self_state_dim)
    target_net = LstmValueNet(trainer.state_dict(), device=dev, self_state_dim=trainer.self_state_dim)  # explorer.update_target_model
    policy = DeviceSarlPolicy(net, actions, gamma) if om is None else DeviceSarlPolicy(net, actions, gamma, om=om)
    t_max = int(round(env.params.time_limit / env.params.time_step)) + 2
    store = EpisodeStore(env.E, t_max, env.R, width, dev)
    for it in range(int(train_iterations)):
        eps = epsilon_start + (epsilon_end - epsilon_start) / epsilon_decay * it if it < epsilon_decay else epsilon_end
        if om is None:
            mean_r = collect(env, policy, target_net, memory, steps_per_iteration, gamma, epsilon=eps, generator=generator,
                             store=store, state_transform=sort_rows_by_distance)
        else:
            mean_r = collect(env, policy, target_net, memory, steps_per_iteration, gamma, epsilon=eps, generator=generator,
                             store=store, om=om, sorted_rows=True)
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
