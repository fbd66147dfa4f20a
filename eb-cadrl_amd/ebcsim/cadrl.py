"""The CADRL value network and its decision (rl/policy/cadrl.py:24-31, 194-217), batched.

The reference runs `value_network` (a plain four-layer perceptron) on every (robot, other) row of a candidate's next
state SEPARATELY and keeps the minimum over the rows: an action is worth reward + gamma^(dt * v_pref) * min, and the
first action above every earlier one is taken.  A batch here holds joint states of different sizes, so the minimum is
taken over each state's own rows (n_valid) and rows beyond them never enter.

CadrlModule is the torch module (the reference's state_dict keys: its .pth files load as they are).  CadrlValueNet is
the inference view with the surface DeviceSarlPolicy and evaluate() drive: on a HIP device the rows go through the
two-layer blocks' float32 form (ebc_mlp2_forward_f32) and the reduction and the decision are one kernel
(ebc_cadrl_decide); on the CPU it is torch."""
import torch

from . import _abi
from .lstm_rl import _sequential, _stack
from .mlp2 import Mlp2Block
from .sarl import DeviceSarlPolicy


def min_over_rows(v, n_valid=None):
    """torch.min over the rows that exist: v [B, R] -> [B].  A NaN among a state's own rows makes its minimum NaN
    (torch.min propagates it), rows at or past n_valid [B] never enter, and a state with no row gives NaN (the
    reference cannot decide such a state either: its torch.cat of an empty list raises)."""
    if n_valid is None:
        return torch.min(v, dim=1)[0]
    live = torch.arange(v.shape[1], device=v.device)[None, :] < n_valid.to(v.device)[:, None]
    m = torch.min(torch.where(live, v, torch.full_like(v, float("inf"))), dim=1)[0]
    return torch.where(live.any(dim=1), m, torch.full_like(m, float("nan")))


def running_choice(values):
    """cadrl.py:192-217 on values [E, A]: `max_min_value = -inf; if min_value > max_min_value` over the actions in
    order -> the chosen action of every env [E] int64: the first maximum, a NaN never, -1 where no value is above -inf
    (the reference then returns max_action = None)."""
    v = values.masked_fill(torch.isnan(values), float("-inf"))
    choice = torch.argmax(v, dim=1)  # the first maximal index
    return torch.where((v > float("-inf")).any(dim=1), choice, torch.full_like(choice, -1))


class CadrlModule(torch.nn.Module):
    """ValueNetwork of rl/policy/cadrl.py with its parameter names (value_network.{0,2,4,6}.{weight,bias})."""

    def __init__(self, input_dim, mlp_dims):
        super().__init__()
        self.input_dim = int(input_dim)
        self.value_network = _sequential(input_dim, mlp_dims)

    @classmethod
    def from_state_dict(cls, sd):
        """The module a reference state_dict belongs to (its shapes give the widths)."""
        idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("value_network.")})
        m = cls(int(sd["value_network.%d.weight" % idx[0]].shape[1]),
                [int(sd["value_network.%d.weight" % i].shape[0]) for i in idx])
        m.load_state_dict(sd, strict=True)
        return m

    def forward(self, rows, n_valid=None):
        """rows [B, R, T]; n_valid [B] (rows that exist) or None = all -> the minimum over each state's rows [B]."""
        B, R, T = rows.shape
        if T != self.input_dim:
            raise ValueError("CadrlModule: rows are %d wide, the network takes %d" % (T, self.input_dim))
        return min_over_rows(self.value_network(rows.reshape(B * R, T)).reshape(B, R), n_valid)


def native_decide(v, reward, discount, n_valid=None, values=None, choice=None):
    """ebc_cadrl_decide: v [E, A, R] float32 (the network's output per row), reward [E, A] float64 -> (values [E, A]
    float64, choice [E] int32) on v's device."""
    import ctypes as C
    from . import _capi
    E, A, R = v.shape
    v, reward = v.contiguous(), reward.to(torch.float64).contiguous()
    assert v.dtype == torch.float32 and v.is_cuda and tuple(reward.shape) == (E, A) and reward.device == v.device
    if values is None:
        values = torch.empty((E, A), dtype=torch.float64, device=v.device)
    if choice is None:
        choice = torch.empty((E,), dtype=torch.int32, device=v.device)
    assert values.dtype == torch.float64 and values.is_contiguous() and tuple(values.shape) == (E, A)
    assert choice.dtype == torch.int32 and choice.is_contiguous() and tuple(choice.shape) == (E,)
    a = _abi.EbcCadrlArgs()
    a.struct_size = C.sizeof(a)
    a.E, a.A, a.R, a.discount = int(E), int(A), int(R), float(discount)
    a.v, a.reward, a.values, a.choice = v.data_ptr(), reward.data_ptr(), values.data_ptr(), choice.data_ptr()
    keep = None
    if n_valid is not None:
        keep = n_valid.to(device=v.device, dtype=torch.int64).contiguous()
        assert tuple(keep.shape) == (E,)
        a.n_valid = keep.data_ptr()
    _capi.check(_capi.lib().ebc_cadrl_decide(torch.cuda.current_stream(v.device).cuda_stream, C.addressof(a)))
    return values, choice


class CadrlValueNet(object):
    """Inference view of a CADRL value network from the reference's state_dict, with the surface DeviceSarlPolicy uses
    (device, forward, action_values, native_forwards, values_decidable, load)."""

    def __init__(self, state_dict, device="cpu"):
        self.device = torch.device(device)
        self.module = CadrlModule.from_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()}
                                                  ).to(self.device).eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
        self.input_dim = self.module.input_dim
        self.native_forwards = 0
        self.native_refreshes = 0
        self.values_decidable = False
        self.last_choice = None
        self._native = None

    @classmethod
    def load(cls, path, device="cpu", **kw):
        return cls(torch.load(path, map_location="cpu"), device=device, **kw)

    def _native_blocks(self):
        """The network as two two-layer blocks on a HIP device; None on the CPU.  A network the blocks do not take
        (other layer counts, more than one output, widths past the kernels' limits) is an error, never a torch path."""
        if self.device.type != "cuda":
            return None
        if self._native is None:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            layers = _stack(self.module.value_network)
            if len(layers) != 4 or int(layers[-1][0].shape[0]) != 1:
                raise NotImplementedError("CadrlValueNet on a HIP device: value_network is four layers ending in one "
                                          "output (two two-layer blocks)")
            self._native = tuple(Mlp2Block(layers[i:i + 2], idx) for i in (0, 2))
        return self._native

    def refresh_native(self, state_dict_or_trainer):
        """New weights for a network that decides: a state_dict of the reference's keys, or a cadrl_train.CadrlTrainer
        (its master copy, read in place on the device).  The module's parameters take them, and on a HIP device the two
        two-layer blocks are re-packed from them on the device (ebc_mlp2_update, no host copy): the next decide gives the
        bytes of a CadrlValueNet freshly built from the same state_dict.  Returns False when the network has no blocks."""
        sd = state_dict_or_trainer
        if hasattr(sd, "device_state_dict"):
            sd = sd.device_state_dict()
        layers = _stack(self.module.value_network)
        with torch.no_grad():
            for i, (w, b) in zip(sorted({int(k.split(".")[1]) for k in sd if k.startswith("value_network.")}), layers):
                w.copy_(sd["value_network.%d.weight" % i])
                b.copy_(sd["value_network.%d.bias" % i])
        if self.device.type != "cuda":
            return False
        nat = self._native_blocks()
        nat[0].update(layers[0:2])
        nat[1].update(layers[2:4])
        self.native_refreshes += 1
        return True

    def _check_width(self, T):
        if T != self.input_dim:
            raise ValueError("CadrlValueNet: rows are %d wide, the network takes %d (CADRL runs with with_agent_type = 0)"
                             % (T, self.input_dim))

    def _row_values(self, x, nat):
        """x [M, T] float32 on the device -> the network's output per row [M] float32."""
        self.native_forwards += 1
        return nat[1].f32(nat[0].f32(x, True), False).view(-1)

    def forward(self, rows, n_valid=None):
        """rows [B, R, T] float32; n_valid [B] or None = all -> the minimum over each state's rows [B] float32."""
        B, R, T = rows.shape
        self._check_width(T)
        with torch.no_grad():
            nat = self._native_blocks() if rows.is_cuda else None
            if nat is None:
                return self.module(rows.to(self.device, torch.float32), n_valid)
            rows = rows.to(torch.float32).contiguous()
            v = self._row_values(rows.view(B * R, T), nat).view(B, 1, R)
            # 0 + 1 * m: the kernel's minimum itself
            values, _ = native_decide(v, torch.zeros((B, 1), dtype=torch.float64, device=rows.device), 1.0, n_valid)
            return values.view(B).to(torch.float32)

    def action_values(self, rows, reward, discount, n_valid=None, refine=None, chunk_pairs=None, eps=None):
        """reward + discount * min over the rows of V(row) for every candidate action (cadrl.py:207-213): rows
        [E, A, R, T] float32, reward [E, A] float64 -> values [E, A] float64; the choice the same rule makes of them is
        kept as `last_choice` [E] (-1: no value above -inf).  Every value is the float32 network's: `refine` (SARL's
        re-evaluated candidate set) has nothing to do here and is ignored."""
        E, A, R, T = rows.shape
        self._check_width(T)
        with torch.no_grad():
            nat = self._native_blocks() if rows.is_cuda else None
            reward = reward.to(torch.float64)
            if nat is None:
                nv = None if n_valid is None else n_valid.repeat_interleave(A)
                m = self.module(rows.to(self.device, torch.float32).reshape(E * A, R, T), nv).view(E, A)
                values = reward.to(m.device) + float(discount) * m.to(torch.float64)
                self.last_choice = running_choice(values).to(torch.int32)
            else:
                rows = rows.to(torch.float32).contiguous()
                values = torch.empty((E, A), dtype=torch.float64, device=rows.device)
                choice = torch.empty((E,), dtype=torch.int32, device=rows.device)
                step = E if not chunk_pairs else max(1, int(chunk_pairs) // A)
                for e0 in range(0, E, step):
                    e1 = min(E, e0 + step)
                    v = self._row_values(rows[e0:e1].view(-1, T), nat).view(e1 - e0, A, R)
                    native_decide(v, reward[e0:e1], discount, None if n_valid is None else n_valid[e0:e1],
                                  values[e0:e1], choice[e0:e1])
                self.last_choice = choice
        self.values_decidable = False  # whether an env has a value above -inf is known on the device alone: last_choice
        return values


class DeviceCadrlPolicy(DeviceSarlPolicy):
    """DeviceSarlPolicy around a CadrlValueNet that takes the decision kernel's own choice instead of an argmax over
    the values: no second pass over them and no host round trip.  An env with no value above -inf (the reference
    returns no action there) gets a NaN action."""

    def choose(self, values):
        return self.net.last_choice.to(torch.int64)

    def decide(self, env, human_policy=_abi.HUMAN_ORCA):
        actions, values = DeviceSarlPolicy.decide(self, env, human_policy)
        undecided = (self.net.last_choice < 0)[:, None]
        return torch.where(undecided, torch.full_like(actions, float("nan")), actions), values
