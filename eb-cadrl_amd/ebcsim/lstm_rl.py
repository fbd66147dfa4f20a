"""The LSTM-RL value networks (rl/policy/lstm_rl.py:9-69), batched.

ValueNetwork1: rows -> nn.LSTM(input_dim, H) -> mlp([self_state | h_n]); ValueNetwork2 (with_interaction_module): rows ->
mlp1 (four layers, no ReLU on the last) -> nn.LSTM(mlp1_dims[-1], H) -> mlp.  h0 = c0 = 0, self_state = the first
self_state_dim columns of row 0, the value is mlp's one output.  The reference runs the LSTM over every row it built;
a batch here holds joint states of different sizes, so h_n is taken at each state's own length (n_valid) and rows
beyond it never enter.

LstmModule is the torch module (state_dict keys and shapes of the reference's networks: their .pth files load as they
are).  LstmValueNet is the inference view with the surface DeviceSarlPolicy and evaluate() drive: on a HIP device every
value is float32 from the library — the two-layer blocks' float32 form (ebc_mlp2_forward_f32) around the LSTM scan
kernel (ebc_lstm_forward), which also writes the joint vector; on the CPU it is torch.  OM-LSTM (with_om = true) is the
same two networks on rows 13 + W wide, up to the kernels' 64 columns."""
import torch

from . import _abi
from .mlp2 import Mlp2Block
from .sarl import chunk_values


def _sequential(input_dim, dims):
    """rl/policy/cadrl.py:13-21 with last_relu = False: Linear at the even indices, ReLU between."""
    layers, dims = [], [input_dim] + list(dims)
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i != len(dims) - 2:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


def _stack(seq):
    return [(m.weight, m.bias) for m in seq if isinstance(m, torch.nn.Linear)]


def masked_lstm(lstm, x, n_valid=None):
    """h_n [B, H] of nn.LSTM `lstm` on x [B, R, I] with h0 = c0 = 0, taken at each sequence's own length n_valid [B]
    (None = R; 0 leaves h_n = 0).  A loop over the rows that keeps h and c by selection past a sequence's end: rows
    beyond it (NaN included) never reach the result."""
    B, R, _ = x.shape
    H = lstm.hidden_size
    w_ih, w_hh, b = lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0
    h = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    c = torch.zeros_like(h)
    for t in range(R):
        pre = torch.addmm(b, x[:, t], w_ih.t()) + h @ w_hh.t()
        i, f, g, o = pre.split(H, dim=1)
        c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h_new = torch.sigmoid(o) * torch.tanh(c_new)
        if n_valid is None:
            h, c = h_new, c_new
        else:
            live = (n_valid > t)[:, None]
            h, c = torch.where(live, h_new, h), torch.where(live, c_new, c)
    return h


class LstmModule(torch.nn.Module):
    """ValueNetwork1 (mlp1_dims None) / ValueNetwork2 of rl/policy/lstm_rl.py with their parameter names."""

    def __init__(self, input_dim, self_state_dim, mlp_dims, lstm_hidden_dim, mlp1_dims=None):
        super().__init__()
        self.input_dim = int(input_dim)
        self.self_state_dim = int(self_state_dim)
        self.lstm_hidden_dim = int(lstm_hidden_dim)
        if mlp1_dims is not None:
            self.mlp1 = _sequential(input_dim, mlp1_dims)
        self.mlp = _sequential(self_state_dim + lstm_hidden_dim, mlp_dims)
        self.lstm = torch.nn.LSTM(mlp1_dims[-1] if mlp1_dims is not None else input_dim, lstm_hidden_dim, batch_first=True)

    @property
    def with_interaction_module(self):
        return hasattr(self, "mlp1")

    @classmethod
    def from_state_dict(cls, sd, self_state_dim=6):
        """The module a reference state_dict belongs to (its shapes say which network it is)."""
        def dims(prefix):
            idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith(prefix + ".")})
            return [int(sd["%s.%d.weight" % (prefix, i)].shape[0]) for i in idx]
        H = int(sd["lstm.weight_hh_l0"].shape[1])
        two = any(k.startswith("mlp1.") for k in sd)
        input_dim = int(sd["mlp1.0.weight"].shape[1]) if two else int(sd["lstm.weight_ih_l0"].shape[1])
        m = cls(input_dim, self_state_dim, dims("mlp"), H, dims("mlp1") if two else None)
        m.load_state_dict(sd, strict=True)
        return m

    def forward(self, rows, n_valid=None):
        """rows [B, R, T]; n_valid [B] (rows that exist) or None = all -> values [B, 1] (the reference's shape)."""
        B, R, T = rows.shape
        if T != self.input_dim:
            raise ValueError("LstmModule: rows are %d wide, the network takes %d" % (T, self.input_dim))
        self_state = rows[:, 0, :self.self_state_dim]
        x = self.mlp1(rows.reshape(B * R, T)).reshape(B, R, -1) if self.with_interaction_module else rows
        if n_valid is None:
            h_n = self.lstm(x)[1][0].squeeze(0)  # the reference's own call (h0 = c0 = 0 is nn.LSTM's default)
        else:
            h_n = masked_lstm(self.lstm, x, n_valid)
        return self.mlp(torch.cat([self_state, h_n], dim=1))


class _NativeLstm(object):
    """The LSTM scan on the device (libebcsim ebc_lstm_*)."""

    def __init__(self, lstm, device_index):
        import ctypes as C
        from . import _capi
        self._L, self._C = _capi.lib(), C
        self.I, self.H = int(lstm.input_size), int(lstm.hidden_size)
        host = [t.detach().to("cpu", torch.float32).contiguous().numpy()
                for t in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]
        self._h = C.c_void_p()
        _capi.check(self._L.ebc_lstm_create(int(device_index), self.I, self.H, host[0].ctypes.data, host[1].ctypes.data,
                                            host[2].ctypes.data, host[3].ctypes.data, C.byref(self._h)))

    def update(self, lstm):
        """Refresh the packed weights from DEVICE tensors (ebc_lstm_update)."""
        from . import _capi
        t = [x.detach().to(torch.float32).contiguous() for x in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]
        assert tuple(t[0].shape) == (4 * self.H, self.I) and tuple(t[1].shape) == (4 * self.H, self.H) and t[0].is_cuda
        _capi.check(self._L.ebc_lstm_update(self._h, torch.cuda.current_stream(t[0].device).cuda_stream, t[0].data_ptr(),
                                            t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr()))

    def __call__(self, x, B, R, n_valid=None, self_src=None, self_stride=0, self_cols=0, out=None, out_offset=None):
        """x [B * R, I] float32 -> out [B, out_stride] with h_n at out[:, out_offset:out_offset + H] and, with self_src
        (a tensor whose sequence b starts self_stride floats after sequence b - 1), its first self_cols floats in front."""
        from . import _capi
        x = x.contiguous()
        assert x.dtype == torch.float32 and x.numel() == B * R * self.I, (tuple(x.shape), B, R, self.I)
        off = int(self_cols if out_offset is None else out_offset)
        if out is None:
            out = torch.empty((B, off + self.H), dtype=torch.float32, device=x.device)
        assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == B and out.stride(1) == 1
        a = _abi.EbcLstmArgs()
        a.struct_size = self._C.sizeof(a)
        a.B, a.R, a.out_offset, a.self_cols = int(B), int(R), off, int(self_cols if self_src is not None else 0)
        a.out_stride, a.self_stride = int(out.stride(0)), int(self_stride)
        a.x, a.out = x.data_ptr(), out.data_ptr()
        keep = None
        if n_valid is not None:
            keep = n_valid.to(torch.int64).contiguous()
            a.n_valid = keep.data_ptr()
        if self_src is not None:
            a.self_src = self_src.data_ptr()
        _capi.check(self._L.ebc_lstm_forward(self._h, torch.cuda.current_stream(x.device).cuda_stream, self._C.addressof(a)))
        return out

    def __del__(self):
        try:
            self._L.ebc_lstm_destroy(self._h)
        except Exception:
            pass


class LstmValueNet(object):
    """Inference view of an LSTM-RL value network from the reference's state_dict, with the surface DeviceSarlPolicy
    uses (device, forward, action_values, native_forwards, load)."""

    def __init__(self, state_dict, device="cpu", self_state_dim=6):
        self.device = torch.device(device)
        self.module = LstmModule.from_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()},
                                                 self_state_dim).to(self.device).eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
        self.input_dim = self.module.input_dim
        self.self_state_dim = self.module.self_state_dim
        self.native_forwards = 0
        self.native_refreshes = 0
        self.values_decidable = False
        self._native = None

    @classmethod
    def load(cls, path, device="cpu", **kw):
        return cls(torch.load(path, map_location="cpu"), device=device, **kw)

    MAX_INPUT_DIM = 64  # csrc/ebc_lstm_cell.h EBC_LSTM_MAX_DIM (the scan), csrc/ebc_lstm_grad_rule.h EBC_LSTM_GRAD_MAX_IN (training)

    def check_native_width(self):
        """The row width the library's LSTM path takes: 13 (LSTM-RL), 13 + W up to 64 (OM-LSTM: 61 at the reference's [om]),
        with mlp1 and without (ValueNetwork1: the cell's own input is that wide).  A wider network is refused by name."""
        if self.input_dim > self.MAX_INPUT_DIM:
            raise NotImplementedError("LstmValueNet on a HIP device: rows %d wide, the LSTM kernels take rows up to %d wide "
                                      "(EBC_LSTM_MAX_DIM, EBC_LSTM_GRAD_MAX_IN)" % (self.input_dim, self.MAX_INPUT_DIM))

    def _native_blocks(self):
        """(mlp1 as two blocks or (), the LSTM, mlp as two blocks) on a HIP device; None on the CPU.  A network the
        blocks do not take (other layer counts, widths past the kernels' limits) is an error, never a torch path."""
        if self.device.type != "cuda":
            return None
        if self._native is None:
            self.check_native_width()
            m = self.module
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            mlp, mlp1 = _stack(m.mlp), (_stack(m.mlp1) if m.with_interaction_module else [])
            if len(mlp) != 4 or len(mlp1) not in (0, 4) or int(mlp[-1][0].shape[0]) != 1:
                raise NotImplementedError("LstmValueNet on a HIP device: mlp1 and mlp are four layers each (two two-layer blocks)")
            pre = tuple(Mlp2Block(mlp1[i:i + 2], idx) for i in (0, 2)) if mlp1 else ()
            self._native = (pre, _NativeLstm(m.lstm, idx), tuple(Mlp2Block(mlp[i:i + 2], idx) for i in (0, 2)))
        return self._native

    def refresh_from(self, state_dict_or_trainer):
        """New weights for a network that decides: a state_dict of the reference's keys, or a lstm_train.LstmTrainer (its
        master copy, read in place on the device).  They are copied into the module's tensors; on a HIP device the float32
        two-layer blocks (Mlp2Block.update) and the scan's packed weights (_NativeLstm.update) are then re-packed from
        them on the device, and native_refreshes counts it.  The decisions afterwards are a freshly built LstmValueNet's.
        Returns whether there were blocks to re-pack."""
        sd = state_dict_or_trainer
        if hasattr(sd, "device_state_dict"):
            sd = sd.device_state_dict()
        with torch.no_grad():
            for k, p in self.module.state_dict().items():
                p.copy_(sd[k])
        nat = self._native_blocks()
        if nat is None:
            return False
        m = self.module
        pre, lstm, post = nat
        for blocks, layers in ((pre, _stack(m.mlp1) if pre else []), (post, _stack(m.mlp))):
            for i, blk in enumerate(blocks):
                blk.update(layers[2 * i:2 * i + 2])
        lstm.update(m.lstm)
        self.native_refreshes += 1
        return True

    def forward(self, rows, n_valid=None):
        """rows [B, R, T] float32; n_valid [B] or None = all -> values [B] float32."""
        B, R, T = rows.shape
        if T != self.input_dim:
            raise ValueError("LstmValueNet: rows are %d wide, the network takes %d (LSTM-RL runs with with_agent_type = 0; "
                             "OM-LSTM's rows carry their maps)" % (T, self.input_dim))
        with torch.no_grad():
            nat = self._native_blocks() if rows.is_cuda else None
            if nat is None:
                return self.module(rows.to(self.device, torch.float32), n_valid).squeeze(1)
            self.native_forwards += 1
            pre, lstm, post = nat
            rows = rows.to(torch.float32).contiguous()
            x = rows.view(B * R, T)
            if pre:
                x = pre[1].f32(pre[0].f32(x, True), False)
            joint = lstm(x, B, R, n_valid, self_src=rows, self_stride=R * T, self_cols=self.self_state_dim)
            return post[1].f32(post[0].f32(joint, True), False).squeeze(1)

    def action_values(self, rows, reward, discount, n_valid=None, refine=None, chunk_pairs=None, eps=None):
        """reward + discount * V(rows) for every candidate action (multi_human_rl.py:72-76): rows [E, A, R, T] float32,
        reward [E, A] float64 -> values [E, A] float64.  Every value is the float32 network's: `refine` (SARL's
        re-evaluated candidate set) has nothing to do here and is ignored."""
        v, _ = chunk_values(self.forward, rows, n_valid, chunk_pairs)
        self.values_decidable = False  # the reference's rule (NaN never chosen, no value above -inf raises) decides
        return reward.to(torch.float64) + float(discount) * v.to(torch.float64)
