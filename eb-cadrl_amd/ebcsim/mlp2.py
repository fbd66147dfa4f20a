"""The two-layer value-network block on the device (libebcsim ebc_mlp2_*) and the per-pair kernels that sit between
the blocks of a SARL network (ebc_pair_*): plain wrappers, one library call each, on the caller's current stream."""
import ctypes as C

import torch

from . import _abi, _capi


def _out(out, shape, dtype, device):
    """A wrapper's output: `out` when the caller passes one (checked: shape, dtype, contiguous), else a new tensor."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous(), (tuple(out.shape), shape, out.dtype)
    return out


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class Mlp2Block(object):
    """A two-layer block on the bf16 matrix cores with split operands (libebcsim ebc_mlp2_*)."""

    WIDE_MAX = _abi.MLP_WIDE_MAX  # K0, H, O of a wide block (ebc_mlp2_create_wide)
    WIDE_ROWS_PER_WORKGROUP = 256  # rows a workgroup of the wide block's kernel owns (EBC_VNW_ROWS)

    @staticmethod
    def fits(K0, H, O):
        """What ebc_mlp2_create_ex takes: inputs and outputs of up to 7 tiles, a hidden layer of up to 10."""
        return 1 <= K0 <= 224 and 1 <= H <= 320 and 1 <= O <= 224

    @staticmethod
    def fits_wide(K0, H, O):
        """What ebc_mlp2_create_wide takes."""
        return all(1 <= d <= Mlp2Block.WIDE_MAX for d in (K0, H, O))

    @staticmethod
    def has_tile_epilogue(K0, O, wide=False):
        """What ebc_mlp2_forward_reduce / _ex ask of a block whose rows leave through the tile epilogue (partial sums,
        fragments): O a multiple of 4 and more than 1 + 1 tiles (the smallest block has no LDS tile per wave to park one);
        a wide block has none."""
        return not wide and O % 4 == 0 and (K0 + 31) // 32 + (O + 31) // 32 >= 3

    def __init__(self, layers, device_index, final=None, in_fragments=False, wide=False):
        """layers: [(w1, b1), (w2, b2)]; final: optional (w3 [1, O], b3 [1]) third layer with one output.
        in_fragments: the block's input is the fragment tensor another block left with `frag_out` (ebc_mlp2_forward_ex).
        wide: the wide block (ebc_mlp2_create_wide: K0, H, O up to 640; rows in, rows out — no fragments, no tile
        epilogue: reduce and forward_ex with those arguments raise the library's error)."""
        (w1, b1), (w2, b2) = layers
        self._L = _capi.lib()
        self.K0, self.H, self.O = int(w1.shape[1]), int(w1.shape[0]), int(w2.shape[0])
        host = [t.detach().to("cpu", torch.float32).contiguous().numpy() for t in (w1, b1, w2, b2)]
        self.has_final = final is not None
        if final is not None:
            host += [final[0].detach().to("cpu", torch.float32).reshape(-1).contiguous().numpy(),
                     final[1].detach().to("cpu", torch.float32).reshape(-1).contiguous().numpy()]
        self._h = C.c_void_p()
        self.in_fragments = bool(in_fragments)
        self.wide = bool(wide)
        self.tile_epilogue = self.has_tile_epilogue(self.K0, self.O, wide)
        create = self._L.ebc_mlp2_create_wide if wide else self._L.ebc_mlp2_create_ex  # (the wide entry refuses in_fragments)
        _capi.check(create(int(device_index), self.K0, self.H, self.O, host[0].ctypes.data,
                           host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data,
                           host[4].ctypes.data if final is not None else None,
                           host[5].ctypes.data if final is not None else None,
                           _abi.MLP_IN_FRAGMENTS if in_fragments else 0, C.byref(self._h)))

    @staticmethod
    def frag_buffer(M, width, device):
        """Storage for an [M, width] activation handed on in fragment order: [row tiles][column tiles][2][2][64] x 16 B."""
        return torch.empty(((M + 31) // 32, (width + 31) // 32, 2, 2, 64, 4), dtype=torch.int32, device=device)

    def _rows(self, entry, x, relu_out, row_bias, group_rows, out):
        """Rows in, rows out through `entry` (ebc_mlp2_forward or its float32 twin: the same arguments)."""
        x = x.contiguous()
        y = _out(out, (x.shape[0],) if self.has_final else (x.shape[0], self.O), torch.float32, x.device)
        if row_bias is not None:
            row_bias = row_bias.contiguous()
        _capi.check(entry(self._h, _stream(x.device), x.data_ptr(), int(x.shape[0]), int(bool(relu_out)), _ptr(row_bias),
                          int(group_rows), y.data_ptr()))
        return y

    def __call__(self, x, relu_out, row_bias=None, group_rows=0, out=None):
        return self._rows(self._L.ebc_mlp2_forward, x, relu_out, row_bias, group_rows, out)

    def f32(self, x, relu_out, row_bias=None, group_rows=0, out=None):
        """The same block in plain float32 on the vector ALUs (ebc_mlp2_forward_f32): float32-GEMM-grade values for the
        few rows that decide an argmax."""
        return self._rows(self._L.ebc_mlp2_forward_f32, x, relu_out, row_bias, group_rows, out)

    def _epilogue_io(self, M, dev, x, row_weight, y_shape, y_out, want_partial, partial_out):
        """What reduce and forward_ex share: contiguous inputs and the outputs that were asked for (y_shape None: no rows)
        -> (x, row_weight, y or None, partial or None)."""
        x = None if x is None else x.contiguous()
        row_weight = None if row_weight is None else row_weight.contiguous()
        y = None if y_shape is None else _out(y_out, y_shape, torch.float32, dev)
        partial = _out(partial_out, ((M + 31) // 32, 3, self.O), torch.float64, dev) if want_partial else None
        return x, row_weight, y, partial

    def forward_ex(self, M, relu_out, x=None, frag_in=None, row_bias=None, group_rows=0, want_y=True, seg_rows=0,
                   row_weight=None, want_partial=False, frag_out=None, general=False, y_out=None, partial_out=None):
        """Every form of the forward in one call (ebc_mlp2_forward_ex): rows or fragments in; rows, per-group partial
        sums and / or fragments out.  -> (y or None, partial or None); y_out / partial_out: the caller's buffers."""
        dev = (x if x is not None else frag_in).device
        y_shape = ((M,) if self.has_final else (M, self.O)) if want_y else None
        x, row_weight, y, partial = self._epilogue_io(M, dev, x, row_weight, y_shape, y_out, want_partial, partial_out)
        if row_bias is not None:
            row_bias = row_bias.contiguous()
        a = _abi.EbcMlpArgs()
        a.struct_size = C.sizeof(a)
        a.M, a.relu_out, a.group_rows, a.seg_rows = int(M), int(bool(relu_out)), int(group_rows), int(seg_rows)
        a.flags = _abi.MLP_GENERAL_KERNEL if general else 0  # the general block where a specialised kernel exists
        for name, t in (("x", x), ("frag_in", frag_in), ("row_bias", row_bias), ("row_weight", row_weight), ("y", y),
                        ("partial", partial), ("frag_out", frag_out)):
            if t is not None:
                setattr(a, name, t.data_ptr())
        _capi.check(self._L.ebc_mlp2_forward_ex(self._h, _stream(dev), C.addressof(a)))
        return y, partial

    def reduce(self, x, relu_out, seg_rows, row_weight=None, store=True):
        """The block with the row-group sums folded into its epilogue (ebc_mlp2_forward_reduce): -> (y or None,
        partial [ceil(M / 32)][3][O]) — ebc_pair_combine turns the partials into per-pair means / weighted sums."""
        M = int(x.shape[0])
        x, row_weight, y, partial = self._epilogue_io(M, x.device, x, row_weight, (M, self.O) if store else None, None,
                                                      True, None)
        _capi.check(self._L.ebc_mlp2_forward_reduce(self._h, _stream(x.device), x.data_ptr(), M, int(bool(relu_out)), None, 0,
                                                    _ptr(y), int(seg_rows), _ptr(row_weight), partial.data_ptr()))
        return y, partial

    def update(self, layers, final=None):
        """Refresh the packed weights from DEVICE tensors of the shapes the block was created with (ebc_mlp2_update)."""
        (w1, b1), (w2, b2) = layers
        t = [x.detach().to(torch.float32).contiguous() for x in (w1, b1, w2, b2)]
        assert tuple(t[0].shape) == (self.H, self.K0) and tuple(t[2].shape) == (self.O, self.H) and t[0].is_cuda
        f = [None, None]
        if final is not None:
            f = [final[0].detach().to(torch.float32).reshape(-1).contiguous(), final[1].detach().to(torch.float32).reshape(-1).contiguous()]
        _capi.check(self._L.ebc_mlp2_update(self._h, _stream(t[0].device), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                            t[3].data_ptr(), _ptr(f[0]), _ptr(f[1])))

    def __del__(self):
        try:
            self._L.ebc_mlp2_destroy(self._h)
        except Exception:
            pass


def pair_mean(h1, nv64, B, R, out=None):
    """sarl.py:56-58 in one pass over h1 (libebcsim ebc_pair_mean)."""
    h1 = h1.contiguous()
    g = _out(out, (B, h1.shape[1]), torch.float32, h1.device)
    _capi.check(_capi.lib().ebc_pair_mean(_stream(h1.device), h1.data_ptr(), _ptr(nv64), B, R, int(h1.shape[1]), g.data_ptr()))
    return g


def pair_attend(scores, feat, nv64, B, R, out=None):
    """sarl.py:69-76 in one pass over the features (libebcsim ebc_pair_attend)."""
    scores, feat = scores.contiguous(), feat.contiguous()
    out = _out(out, (B, feat.shape[2]), torch.float32, feat.device)
    _capi.check(_capi.lib().ebc_pair_attend(_stream(feat.device), scores.data_ptr(), feat.data_ptr(), _ptr(nv64), B, R,
                                            int(feat.shape[2]), out.data_ptr()))
    return out


def pair_combine(partial, nv64, B, R, mean, out=None):
    """Per-pair sums of a block's tile partials (libebcsim ebc_pair_combine): the pair mean (sarl.py:56-58) or,
    with the attention weights as row weights, the weighted feature sum (sarl.py:73-76)."""
    O = int(partial.shape[2])
    out = _out(out, (B, O), torch.float32, partial.device)
    _capi.check(_capi.lib().ebc_pair_combine(_stream(partial.device), partial.data_ptr(), _ptr(nv64), B, R, O, int(bool(mean)),
                                             out.data_ptr()))
    return out


def pair_weights(scores, nv64, B, R):
    """softmax' of the pair's scores (sarl.py:69-71) as row weights [B * R] (libebcsim ebc_pair_weights)."""
    scores = scores.contiguous()
    w = torch.empty((B * R,), dtype=torch.float32, device=scores.device)
    _capi.check(_capi.lib().ebc_pair_weights(_stream(scores.device), scores.data_ptr(), _ptr(nv64), B, R, w.data_ptr()))
    return w


def pair_mask(nv64, B, R):
    """1 for the rows of a pair that exist, else 0, as row weights [B * R] (libebcsim ebc_pair_mask)."""
    w = torch.empty((B * R,), dtype=torch.float32, device=nv64.device)
    _capi.check(_capi.lib().ebc_pair_mask(_stream(nv64.device), nv64.data_ptr(), B, R, w.data_ptr()))
    return w
