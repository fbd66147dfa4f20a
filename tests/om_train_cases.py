"""Shared by tests/test_om_train_cpu.py and tests/test_om_train_gpu.py: the golden of the stored OM-SARL state
(tests/golden/om_train_states.npz: the reference's own SARL.transform with with_om = true), the host build of the SARL
gradient rule on wide rows (tests/native/sarl_grad_om_host.cc: the source the kernel compiles, built with g++), the wide
networks and batches, and the accuracy table both the test and profiles/om_grad_accuracy.txt come from.

A wide network is ((widths, self_state_dim, with_global_state), om_width): widths[0] = T + om_width is what mlp1's first
layer takes (the shape ebcsim.sarl_train.shape_of reads off a state_dict), T = widths[0] - om_width the rotated width.

Bar of the gradient.  The project's (tests/sarl_grad_cases.py): per layer err = max |g - g_64| / max |g_64| against float64
autograd of the wide SarlModule on the same float32 weights and inputs, within TOL_FACTOR (8) times torch's own float32
error; where torch's error of a layer is below 2^-25 (half a unit of float32's last place: no float32 result can be held
to a multiple of less) the bar is 8 x 2^-25, the rule profiles/lstm_grad_accuracy.txt set.  The batches are fixed by
their seeds; the precondition (in float64 no score exactly 0 and no softmax denominator 0) is asserted, not searched for."""
import ctypes as C
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

import sarl_grad_cases as sg
from cadrl_cases import TOL_FACTOR  # noqa: F401
from ebcsim.occupancy import OccupancySpec
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "sarl_grad_om_host.cc")
YARDSTICK_FLOOR = 2.0 ** -25
NARROW_UNITS = sg.NARROW_WIDTHS[1:]
REFERENCE_UNITS = sg.REFERENCE_WIDTHS[1:]
# (rotated width T, om_width W): the reference's own OM config on both row widths (61, 65) and the limit T + W = 224
WIDE_SHAPES = [(13, 48), (17, 48), (32, 192)]
BATCHES = sg.BATCHES


def wide_net(T, W, units=NARROW_UNITS, glob=True, self_dim=6):
    return (([T + W] + list(units), self_dim, glob), W)


NARROW_WIDE = [wide_net(T, W) for T, W in WIDE_SHAPES]
REFERENCE_WIDE_65 = wide_net(17, 48, REFERENCE_UNITS)

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/sarl_grad_om_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="sarl_grad_om_host_")
        L = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libsarl_grad_om_host.so")))
        for name in ("max_om", "max_wide", "max_row"):
            getattr(L, "sarl_grad_om_host_" + name).restype = C.c_int
        L.sarl_grad_om_host_refused.restype, L.sarl_grad_om_host_refused.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]
        L.sarl_grad_om_host_floats.restype, L.sarl_grad_om_host_floats.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.sarl_grad_om_host_pack.restype, L.sarl_grad_om_host_pack.argtypes = None, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.sarl_grad_om_host.restype = None
        L.sarl_grad_om_host.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float]
                                        + [C.c_void_p] * 5)
        _host["lib"] = L
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="sarl_grad_om_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "sarl_grad_om_host"))
    return _host[key]


def rotated_widths(wnet):
    """The widths the OM entries take: [0] the rotated width T."""
    (widths, _, _), W = wnet
    return np.ascontiguousarray([widths[0] - W] + list(widths[1:]), dtype=np.int32)


def host_refused(widths_rotated, self_dim, om_width):
    w = np.ascontiguousarray(widths_rotated, dtype=np.int32)
    return int(host_lib().sarl_grad_om_host_refused(w.ctypes.data, int(self_dim), int(om_width)))


def host_floats(wnet):
    (_, S, glob), W = wnet
    w = rotated_widths(wnet)
    return int(host_lib().sarl_grad_om_host_floats(w.ctypes.data, S, int(glob), W))


def host_pack(sd, om_width):
    """The packed image of a wide state_dict by the header's own pack."""
    from ebcsim.sarl_train import LAYER_KEYS, shape_of
    wnet = (shape_of(sd), om_width)
    w = [np.ascontiguousarray(sd[k + ".weight"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    b = [np.ascontiguousarray(sd[k + ".bias"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    P = np.full(host_floats(wnet), -7.0, dtype=np.float32)
    wp, bp, wd = (C.c_void_p * 11)(*[a.ctypes.data for a in w]), (C.c_void_p * 11)(*[a.ctypes.data for a in b]), rotated_widths(wnet)
    host_lib().sarl_grad_om_host_pack(wd.ctypes.data, wnet[0][1], int(wnet[0][2]), om_width, wp, bp, P.ctypes.data)
    return P


def host_grad(P, wnet, rows, target, n_valid=None, mask=None, grad_scale=1.0):
    """(grad float32 [packed floats], loss_sum, count, value [B] float32, attention [B, R] float32) of the host build."""
    (widths, S, glob), W = wnet
    rows, target = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    B, R, T = rows.shape
    assert T == widths[0] and target.shape == (B,)
    P = np.ascontiguousarray(P, dtype=np.float32)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    grad = np.full(P.shape, -7.0, dtype=np.float32)
    loss, count = C.c_double(-1.0), C.c_longlong(-1)
    value, att, wd = np.full((B,), -7.0, dtype=np.float32), np.full((B, R), -7.0, dtype=np.float32), rotated_widths(wnet)
    host_lib().sarl_grad_om_host(wd.ctypes.data, S, int(glob), W, P.ctypes.data, B, R, rows.ctypes.data, None if nv is None else nv.ctypes.data,
                                 target.ctypes.data, None if mk is None else mk.ctypes.data, float(grad_scale), grad.ctypes.data,
                                 C.addressof(loss), C.addressof(count), value.ctypes.data, att.ctypes.data)
    return grad, float(loss.value), int(count.value), value, att


def write_batches(path, batch_list):
    """The input file of the host program (the format is in sarl_grad_om_host.cc): batches of (wide net, P, rows, target,
    n_valid or None, mask or None, grad_scale)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batch_list)))
        for wnet, P, rows, target, nv, mk, scale in batch_list:
            (_, S, glob), W = wnet
            B, R, _ = rows.shape
            f.write(struct.pack("<19if", *rotated_widths(wnet).tolist(), S, int(glob), B, R, int(nv is not None), int(mk is not None), W,
                                float(scale)))
            f.write(np.ascontiguousarray(P, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(target, dtype="<f4").tobytes())
            if mk is not None:
                f.write(np.ascontiguousarray(mk, dtype="u1").tobytes())


read_results = sg.read_results
same_bytes = sg.same_bytes


def same_results(a, b):
    return (same_bytes(a[0], b[0]) and struct.pack("<d", a[1]) == struct.pack("<d", b[1]) and a[2] == b[2] and same_bytes(a[3], b[3])
            and same_bytes(a[4], b[4]))


def wide_batch(wnet, B, R, seed):
    """(rows [B, R, T + W] float32, target [B]): the first T columns like rotated joint states in size, the map columns
    like maps: mostly 0, some occupancy ones, some mean velocities."""
    (widths, _, _), W = wnet
    T = widths[0] - W
    rs = np.random.RandomState(seed)
    rows = rs.normal(0.0, 1.0, (B, R, T + W)).astype(np.float32)
    m = rows[:, :, T:]
    kind = rs.uniform(size=m.shape)
    m[kind < 0.6] = 0.0
    m[(kind >= 0.6) & (kind < 0.8)] = 1.0
    return rows, rs.normal(0.0, 0.5, (B,)).astype(np.float32)


def ragged_masked(B, R, seed):
    """n_valid [B] in 1 .. R with the first state ragged (R > 1) and, from B = 3 on, one masked state."""
    rs = np.random.RandomState(seed)
    nv = rs.randint(1, R + 1, size=B).astype(np.int64)
    if R > 1:
        nv[0] = R - 1
    mask = np.ones(B, dtype=np.uint8)
    if B >= 3:
        mask[1] = 0
    return nv, mask


# (wide net index into ACCURACY_NETS, B, R): T + W = 61, 65 and 224, both values of with_global_state
ACCURACY_NETS = NARROW_WIDE + [wide_net(17, 48, glob=False), wide_net(32, 192, glob=False), REFERENCE_WIDE_65]
ACCURACY_CASES = [(0, 9, 5), (1, 9, 5), (2, 9, 5), (3, 9, 5), (4, 5, 3), (5, 9, 5)]
_rows = {}


def accuracy_row(ni, B, R):
    """Per compared layer (name, err_rule, err_torch32, bar), the loss's likewise, and the precondition (smallest |score|
    and smallest softmax denominator in float64) of one seeded batch with ragged n_valid and a masked state."""
    if (ni, B, R) not in _rows:
        from ebcsim.sarl_train import LAYER_KEYS
        wnet = ACCURACY_NETS[ni]
        net, W = wnet
        sd = sg.random_state_dict(net)
        seed = 810000 + 1000 * ni + 10 * B + R
        rows, target = wide_batch(wnet, B, R, seed)
        nv, mask = ragged_masked(B, R, seed + 1)
        live = sg.is_live(nv, mask)
        scale = 2.0 / live.sum()
        s64, den64, _, _ = sg.torch_scores(sd, rows, nv, torch.float64)
        valid = np.arange(R)[None, :] < nv[:, None]
        g64, l64, _ = sg.torch_grad(sd, rows, target, nv, live, scale, torch.float64)
        g32, l32, _ = sg.torch_grad(sd, rows, target, nv, live, scale, torch.float32)
        g, loss, count, _, _ = host_grad(host_pack(sd, W), wnet, rows, target, nv, mask, scale)
        assert count == int(live.sum())
        sl = sg.layer_slices(net)
        # a state of one row has softmax weight 1 whatever its score: when every live state is one, attention's exact gradient is 0
        layers_in = [l for l in range(11) if not (l in sg.ATTENTION_LAYERS and (nv[live] == 1).all())]
        assert all(np.abs(g64[sl[l]]).max() > 0 for l in layers_in), "a layer's exact gradient is 0: nothing to take a relative error of"
        err = lambda a, l: float(np.abs(a[sl[l]].astype(np.float64) - g64[sl[l]]).max() / np.abs(g64[sl[l]]).max())  # noqa: E731
        layers = [(LAYER_KEYS[l], err(g, l), err(g32, l), TOL_FACTOR * max(err(g32, l), YARDSTICK_FLOOR)) for l in layers_in]
        lt = abs(l32 - l64) / l64
        _rows[ni, B, R] = (layers, (abs(loss - l64) / l64, lt, TOL_FACTOR * max(lt, YARDSTICK_FLOOR)),
                           (float(np.abs(s64[valid]).min()), float(den64.min())))
    return _rows[ni, B, R]


def net_name(wnet):
    (widths, _, glob), W = wnet
    return "%d+%d-" % (widths[0] - W, W) + "-".join(str(w) for w in widths[1:]) + ("" if glob else " (no global state)")


def accuracy_table():
    lines = ["SARL gradient rule on the wide rows of OM-SARL (csrc/ebc_sarl_grad_rule.h, host build tests/native/sarl_grad_om_host.cc)",
             "against torch autograd of the wide SarlModule in float64, beside torch's own float32 autograd:",
             "err = max |g - g_64| / max |g_64| per layer (W and bias together).  Seeded networks and batches of tests/om_train_cases.py",
             "(ragged n_valid, one masked state); bar: rule <= %d x max(torch32, 2^-25), the floor profiles/lstm_grad_accuracy.txt set;" % TOL_FACTOR,
             "`floor` marks a row whose torch32 error is below 2^-25 (the ratio printed is against torch's error all the same).", ""]
    for i, wnet in enumerate(ACCURACY_NETS):
        lines.append("net %d: %s" % (i, net_name(wnet)))
    lines += ["", "%-4s %4s %3s  %-16s %11s %11s %7s" % ("net", "B", "R", "layer", "err_rule", "err_torch32", "ratio")]
    ratio = lambda a, b: a / b if b else (float("inf") if a else 0.0)  # noqa: E731
    for ni, B, R in ACCURACY_CASES:
        layers, (lr, lt, _), _ = accuracy_row(ni, B, R)
        for key, er, et, _ in layers + [("loss_sum", lr, lt, 0.0)]:
            lines.append("%-4d %4d %3d  %-16s %11.3e %11.3e %7.2f%s" % (ni, B, R, key, er, et, ratio(er, et), "  floor" if et < YARDSTICK_FLOOR else ""))
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------- the golden of the stored state
def golden_states():
    """[(robot [9], ob [R, 5], types [R], T, unicycle, spec, kind name, the reference's transform [R, T + W] float32 — [R, T]
    for a lone row, whose maps the reference cannot build)] of tests/golden/om_train_states.npz, and its meta."""
    if "states" not in _host:
        z = load("om_train_states")
        meta = json.loads(str(z["meta"]))
        out = []
        for i in range(len(z["rows"])):
            R, T = int(z["rows"][i]), int(z["T"][i])
            spec = OccupancySpec(z["cell_num"][i], z["cell_size"][i], z["channels"][i])
            want = z["state"][z["offsets"][i]:z["offsets"][i + 1]].reshape(R, -1)
            out.append((z["robot"][i], np.ascontiguousarray(z["ob"][i, :R]), z["types"][i, :R], T, int(z["unicycle"][i]), spec,
                        meta["kinds"][int(z["kind"][i])], want))
        _host["states"] = (out, meta)
    return _host["states"]


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "om_grad_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
