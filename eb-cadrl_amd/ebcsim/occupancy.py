"""Occupancy maps of OM-SARL: rl/policy/multi_human_rl.py:156-227 (build_occupancy_maps), :62-69 (the maps appended to
every candidate action's rows) and :151-154 (input_dim).

`occupancy_maps` is the rule of csrc/ebc_om_rule.h in numpy float64 — the CPU / oracle backends and `last_state` use it;
`occupancy_rows_device` is the kernel (ebc_occupancy_rows) on torch CUDA tensors.  Both state the reference's
arctan2 / cos / sin frame algebraically: c = vx / |v|, s = vy / |v|, a standing row's frame is (+-1, 0) by the
sign of its vx."""
import collections
import ctypes as C

import numpy as np

from . import _abi

MAX_WIDTH = 192      # cell_num^2 * channels the kernel takes
MAX_ROW_WIDTH = 224  # T + W: the input limit of the two-layer blocks


class OccupancySpec(collections.namedtuple("OccupancySpec", "cell_num cell_size channels")):
    """[om] cell_num / cell_size / om_channel_size of a policy config."""
    __slots__ = ()

    def __new__(cls, cell_num, cell_size, channels):
        cell_num, cell_size, channels = int(cell_num), float(cell_size), int(channels)
        if channels not in (1, 2, 3):
            raise NotImplementedError("om_channel_size %d (multi_human_rl.py:222)" % channels)
        if cell_num < 1 or not (np.isfinite(cell_size) and cell_size > 0):
            raise ValueError("occupancy maps need cell_num >= 1 and a finite positive cell_size")
        return super().__new__(cls, cell_num, cell_size, channels)

    @property
    def width(self):
        """W = cell_num^2 * channels: the columns the maps add to a row."""
        return self.cell_num ** 2 * self.channels

    @classmethod
    def from_config(cls, policy_cfg, section="sarl"):
        """The spec of a policy config in the reference's schema, or None where [section] with_om is false or absent."""
        if not policy_cfg.getboolean(section, "with_om", fallback=False):
            return None
        return cls(policy_cfg.getint("om", "cell_num"), policy_cfg.getfloat("om", "cell_size"),
                   policy_cfg.getint("om", "om_channel_size"))


def occupancy_maps(next_ob, n_valid, spec):
    """next_ob [E, R, >= 4] float64 (px, py, vx, vy, ...), n_valid [E] or None = all R -> maps [E, R, W] float32.  Rows at or
    past n_valid[e] are never read and get zero maps.  The sums of a cell run over its occupants in row order."""
    ob = np.asarray(next_ob, dtype=np.float64)
    E, R = ob.shape[:2]
    n = np.full((E,), R, dtype=np.int64) if n_valid is None else np.clip(np.asarray(n_valid, dtype=np.int64), 0, R)
    exists = np.arange(R)[None, :] < n[:, None]                      # [E, R]
    ob = np.where(exists[:, :, None], ob[:, :, :4], 0.0)             # padding rows are never read
    px, py, vx, vy = (ob[:, :, c] for c in range(4))
    cn, cs, ch = spec.cell_num, spec.cell_size, spec.channels
    with np.errstate(all="ignore"):
        sp = np.sqrt(vx * vx + vy * vy)
        still = sp == 0.0
        safe = np.where(still, 1.0, sp)
        c = np.where(still, np.where(np.signbit(vx), -1.0, 1.0), vx / safe)
        s = np.where(still, 0.0, vy / safe)
        count = np.zeros((E, R, cn * cn), dtype=np.int64)
        sx = np.zeros((E, R, cn * cn))
        sy = np.zeros((E, R, cn * cn))
        ei, ai = np.meshgrid(np.arange(E), np.arange(R), indexing="ij")
        for o in range(R):
            dx, dy = px[:, o:o + 1] - px, py[:, o:o + 1] - py        # [E, R]: occupant o seen from every row a
            x = dx * c + dy * s
            y = dy * c - dx * s
            ix = np.floor(x / cs + 0.5 * cn)
            iy = np.floor(y / cs + 0.5 * cn)
            hit = (ix >= 0) & (ix < cn) & (iy >= 0) & (iy < cn) & exists & exists[:, o:o + 1] & (np.arange(R)[None, :] != o)
            k = np.where(hit, cn * iy + ix, 0).astype(np.int64)
            e_h, a_h, k_h = ei[hit], ai[hit], k[hit]
            count[e_h, a_h, k_h] += 1                                # one occupant per (e, a) here: no index repeats
            if ch > 1:
                ovx, ovy = vx[:, o:o + 1], vy[:, o:o + 1]
                rvx = ovx * c + ovy * s
                rvy = ovy * c - ovx * s
                sx[e_h, a_h, k_h] = sx[e_h, a_h, k_h] + rvx[hit]
                sy[e_h, a_h, k_h] = sy[e_h, a_h, k_h] + rvy[hit]
        filled = count > 0
        occ = filled.astype(np.float32)
        if ch == 1:
            return occ
        div = np.where(filled, count, 1).astype(np.float64)
        mx = np.where(filled, sx / div, 0.0).astype(np.float32)
        my = np.where(filled, sy / div, 0.0).astype(np.float32)
    parts = [mx, my] if ch == 2 else [occ, mx, my]
    return np.stack(parts, axis=3).reshape(E, R, cn * cn * ch)


def boundary_margin(next_ob, n_valid, spec):
    """How close the coordinates of a state come to a cell boundary, in cells: [E, R, R] (row a, occupant o), the smaller
    of the two axes' distance of q = coord / cell_size + cell_num / 2 to the nearest of the grid's boundaries 0 .. cell_num
    (beyond them an occupant is dropped whichever index it gets); inf for a == o and for rows that do not exist.  The algebraic frame and the reference's trigonometric one can differ in the last bits of a coordinate, so
    only a pair whose margin is far above 1e-16 is certain to fall into the same cell in both.  Left out, because the
    coordinate is exact in both forms: coincident pairs (dx = dy = 0: both coordinates are 0 whatever the frame), and
    the axis of a STANDING row along which the occupant's offset is exactly 0 (the frame is (+-1, 0), so the algebraic
    coordinate is +-0, and the reference's is cos(+-pi / 2) or sin(pi) times the distance: a positive 1e-16 that the
    addition of cell_num / 2 absorbs or leaves above the boundary, where +0 lies too) - the wall rows of a generated
    scene stand in axis-aligned pairs."""
    ob = np.asarray(next_ob, dtype=np.float64)
    E, R = ob.shape[:2]
    n = np.full((E,), R, dtype=np.int64) if n_valid is None else np.clip(np.asarray(n_valid, dtype=np.int64), 0, R)
    exists = np.arange(R)[None, :] < n[:, None]
    ob = np.where(exists[:, :, None], ob[:, :, :4], 0.0)
    px, py, vx, vy = (ob[:, :, c] for c in range(4))
    with np.errstate(all="ignore"):
        sp = np.sqrt(vx * vx + vy * vy)
        still = sp == 0.0
        safe = np.where(still, 1.0, sp)
        c = np.where(still, np.where(np.signbit(vx), -1.0, 1.0), vx / safe)[:, :, None]
        s = np.where(still, 0.0, vy / safe)[:, :, None]
        dx, dy = px[:, None, :] - px[:, :, None], py[:, None, :] - py[:, :, None]   # [E, a, o]
        qx = (dx * c + dy * s) / spec.cell_size + 0.5 * spec.cell_num
        qy = (dy * c - dx * s) / spec.cell_size + 0.5 * spec.cell_num
        near = lambda q: np.abs(q - np.clip(np.round(q), 0, spec.cell_num))  # noqa: E731  the grid's own boundaries 0 .. cell_num
        mx = np.where(still[:, :, None] & (dx == 0.0), np.inf, near(qx))
        my = np.where(still[:, :, None] & (dy == 0.0), np.inf, near(qy))
        m = np.minimum(mx, my)
    skip = (~exists[:, :, None]) | (~exists[:, None, :]) | np.eye(R, dtype=bool)[None] | ((dx == 0.0) & (dy == 0.0))
    return np.where(skip, np.inf, m)


def widen(rows, om):
    """rows [..., A, R, T] float32 and om [..., R, W] -> [..., A, R, T + W]: every action's rows with the maps appended
    (multi_human_rl.py:67-69).  numpy arrays or torch tensors."""
    if isinstance(rows, np.ndarray):
        wide = np.broadcast_to(np.asarray(om, dtype=np.float32)[..., None, :, :], rows.shape[:-1] + (om.shape[-1],))
        return np.concatenate([rows, wide], axis=-1)
    import torch
    return torch.cat([rows, om.to(rows.dtype).unsqueeze(-3).expand(*rows.shape[:-1], om.shape[-1])], dim=-1)


def wide_state(rotated, ob, n_valid, spec):
    """The state OM-SARL stores (multi_human_rl.py:128-149 transform = [rotate(state) | build_occupancy_maps(state)]):
    rotated [E, R, T] float32 (the rotated rows of the CURRENT state), ob [E, R, >= 4] float64 (its world-frame rows) and
    n_valid [E] or None -> [E, R, T + W] float32.  Rows at or past n_valid[e] keep their rotated padding and get zero maps.
    `widen` of one "action" over `occupancy_maps`: the CPU path, and the checker of ebc_observe_wide."""
    rotated = np.asarray(rotated, dtype=np.float32)
    return widen(rotated[:, None], occupancy_maps(ob, n_valid, spec))[:, 0]


def observe_wide_composed(env, spec, out=None, n_rows=None):
    """What BatchedEnv.observe_wide_device gives, from the four calls it replaces (ebc_observe twice, ebc_row_counts,
    ebc_occupancy_rows) and a cat: the composition the kernel is held to byte for byte, and measured against."""
    import torch
    dev = torch.device("cuda", env.device)
    rot = torch.empty((env.E, env.R, env.T), dtype=torch.float32, device=dev)
    ob = torch.empty((env.E, env.R, 5), dtype=torch.float64, device=dev)
    n = torch.empty((env.E,), dtype=torch.int64, device=dev) if n_rows is None else n_rows
    env.observe_device(rot)
    env.observe_ob_device(ob)
    env.row_counts_device(n)
    om, _ = occupancy_rows_device(ob, n, spec)
    wide = torch.cat([rot, om], dim=2)
    if out is not None:
        out.copy_(wide)
        return out
    return wide


DISTANCE_COLUMN = 11  # `da` of a rotated row: the sort key of LstmRL.predict's order (lstm_train.DISTANCE_COLUMN)


def distance_order(rotated, n_valid=None):
    """lstm_train.distance_order in numpy: rotated [E, R, >= 12] float32 -> int64 [E, R], each state's existing rows in a
    stable descending order of their float32 column 11 (a NaN behind every number), the padding rows where they are."""
    rotated = np.asarray(rotated, dtype=np.float32)
    E, R = rotated.shape[:2]
    key = -rotated[:, :, DISTANCE_COLUMN]
    key = np.where(np.isnan(key), np.float32(np.inf), key)
    if n_valid is not None:
        n = np.clip(np.asarray(n_valid, dtype=np.int64), 0, R)
        key = np.where(np.arange(R)[None, :] < n[:, None], key, np.float32(np.inf))
    return np.argsort(key, axis=1, kind="stable").astype(np.int64)


def wide_state_sorted(rotated, ob, n_valid, spec):
    """The state OM-LSTM stores in RL: LstmRL.predict sorts the agents by decreasing distance (lstm_rl.py:117-123) and
    transform builds the maps from the SORTED list (multi_human_rl.py:142-146), so a cell's sums walk its occupants in
    that order.  rotated [E, R, T] float32, ob [E, R, >= 4] float64, n_valid [E] or None -> [E, R, T + W] float32:
    both permuted by `distance_order`, then `wide_state`.  The CPU path, and the checker of ebc_observe_wide_sorted."""
    rotated = np.asarray(rotated, dtype=np.float32)
    ob = np.asarray(ob, dtype=np.float64)
    order = distance_order(rotated, n_valid)[:, :, None]
    return wide_state(np.take_along_axis(rotated, order, axis=1), np.take_along_axis(ob, order, axis=1), n_valid, spec)


def observe_wide_sorted_composed(env, spec, n_rows=None):
    """What BatchedEnv.observe_wide_sorted_device gives, from the calls it replaces: ebc_observe twice, ebc_row_counts, a
    torch sort of the distance column and two gathers, ebc_occupancy_rows on the gathered ob, and a cat.  The composition
    the kernel is held to byte for byte, and measured against."""
    import torch
    from .lstm_train import distance_order as order_of
    dev = torch.device("cuda", env.device)
    rot = torch.empty((env.E, env.R, env.T), dtype=torch.float32, device=dev)
    ob = torch.empty((env.E, env.R, 5), dtype=torch.float64, device=dev)
    n = torch.empty((env.E,), dtype=torch.int64, device=dev) if n_rows is None else n_rows
    env.observe_device(rot)
    env.observe_ob_device(ob)
    env.row_counts_device(n)
    order = order_of(rot, n)[:, :, None]
    om, _ = occupancy_rows_device(torch.gather(ob, 1, order.expand_as(ob)).contiguous(), n, spec)
    return torch.cat([torch.gather(rot, 1, order.expand_as(rot)), om], dim=2)


def occupancy_rows_device(next_ob, n_valid, spec, rows=None, om_out=None, wide_out=None, want_om=True):
    """ebc_occupancy_rows on torch CUDA tensors, enqueued on the current stream: next_ob [E, R, 5] float64, n_valid [E]
    int64 or None, rows [E, A, R, T] float32 or None -> (om [E, R, W] or None, rows_wide [E, A, R, T + W] or None).
    om_out / wide_out: the caller's buffers (contiguous, of those shapes)."""
    import torch
    from . import _capi
    from .mlp2 import _out
    dev = next_ob.device
    assert next_ob.dtype == torch.float64 and next_ob.dim() == 3 and next_ob.shape[2] == 5 and next_ob.is_contiguous()
    E, R = int(next_ob.shape[0]), int(next_ob.shape[1])
    a = _abi.EbcOmArgs()
    a.struct_size = C.sizeof(a)
    a.E, a.R = E, R
    a.cell_num, a.cell_size, a.channels = spec.cell_num, spec.cell_size, spec.channels
    a.next_ob = next_ob.data_ptr()
    if n_valid is not None:
        assert n_valid.dtype == torch.int64 and n_valid.is_contiguous() and n_valid.numel() == E
        a.n_valid = n_valid.data_ptr()
    om = wide = None
    if want_om or om_out is not None:
        om = _out(om_out, (E, R, spec.width), torch.float32, dev)
        a.om = om.data_ptr()
    if rows is not None:
        assert rows.dtype == torch.float32 and rows.dim() == 4 and rows.is_contiguous() and rows.shape[0] == E and rows.shape[2] == R
        a.A, a.T = int(rows.shape[1]), int(rows.shape[3])
        a.rows = rows.data_ptr()
        wide = _out(wide_out, (E, a.A, R, a.T + spec.width), torch.float32, dev)
        a.rows_wide = wide.data_ptr()
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    _capi.check(_capi.lib().ebc_occupancy_rows(int(idx), torch.cuda.current_stream(dev).cuda_stream, C.addressof(a)))
    return om, wide
