"""Shared by tests/test_sarl_grad_layers_cpu.py and tests/test_sarl_grad_layers_gpu.py: the WIDE host build of the SARL
gradient rule (tests/native/sarl_grad_layers_host.cc: the rule header with its serial loops' buffers 640 floats a row), the
wide networks, and the accuracy table of profiles/sarl_grad_layers_accuracy.txt.  Batches, edge batches, torch's autograd
and the bar (TOL_FACTOR, `usable` seeds) are tests/sarl_grad_cases.py's, unchanged."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

import sarl_grad_cases as base
from sarl_grad_cases import ROOT, TOL_FACTOR

SOURCE = os.path.join(ROOT, "tests", "native", "sarl_grad_layers_host.cc")
# the row width, then the units of mlp1 (2), mlp2 (2), attention (3), mlp3 (4)
X2_WIDTHS = [17, 300, 200, 200, 100, 200, 200, 1, 300, 200, 200, 1]   # eb-cadrl_amd/configs/policy_x2.config, agent-type rows
X4_WIDTHS = [13, 600, 400, 400, 200, 400, 400, 1, 600, 400, 400, 1]
EDGE_WIDTHS = [17, 33, 64, 65, 31, 32, 63, 1, 95, 34, 2, 1]            # on both sides of the 32- and 64-wide tiles
X2_NET, X4_NET, EDGE_NET = (X2_WIDTHS, 6, True), (X4_WIDTHS, 6, True), (EDGE_WIDTHS, 6, True)
ACCURACY_CASES = [("x2", X2_NET, 9, 5), ("x2", X2_NET, 9, 30), ("x2", X2_NET, 100, 5), ("x4", X4_NET, 9, 5)]

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out], check=True, timeout=300)
    return out


def host_lib():
    """tests/native/sarl_grad_layers_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="sarl_grad_layers_host_")
        L = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libsarl_grad_layers_host.so")))
        for name in ("max_width", "max_rows", "run_slots", "stride", "chunk"):
            getattr(L, "sarl_grad_layers_host_" + name).restype = C.c_int
        for name in ("refused", "refused_chunk"):
            f = getattr(L, "sarl_grad_layers_host_" + name)
            f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]
        L.sarl_grad_layers_host_floats.restype, L.sarl_grad_layers_host_floats.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.sarl_grad_layers_host_layer.restype = None
        L.sarl_grad_layers_host_layer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.sarl_grad_layers_host_pack.restype, L.sarl_grad_layers_host_pack.argtypes = None, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.sarl_grad_layers_host.restype = None
        L.sarl_grad_layers_host.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float]
                                            + [C.c_void_p] * 5)
        _host["lib"] = L
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="sarl_grad_layers_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "sarl_grad_layers_host"))
    return _host[key]


def _w(widths):
    return np.ascontiguousarray(widths, dtype=np.int32)


def constant(name):
    """max_width, max_rows, run_slots, stride or chunk, from the header itself."""
    return int(getattr(host_lib(), "sarl_grad_layers_host_" + name)())


def refused(widths, self_dim=6, om_width=0, chunk_form=False):
    """grad_dims_refused_layers (chunk_form: grad_dims_refused_wide) of the rotated widths."""
    w = _w(widths)
    f = host_lib().sarl_grad_layers_host_refused_chunk if chunk_form else host_lib().sarl_grad_layers_host_refused
    return int(f(w.ctypes.data, int(self_dim), int(om_width)))


def rotated(net, om_width):
    """The widths the host build and the entry take for a network whose rows are net[0][0] wide, om_width of them a map."""
    return [net[0][0] - om_width] + list(net[0][1:])


def host_floats(net, om_width=0):
    w = _w(rotated(net, om_width))
    return int(host_lib().sarl_grad_layers_host_floats(w.ctypes.data, net[1], int(net[2]), int(om_width)))


def layer_slices(net):
    out, w = [], _w(net[0])
    for l in range(11):
        at, k, padded = C.c_longlong(-1), C.c_int(-1), C.c_int(-1)
        host_lib().sarl_grad_layers_host_layer(w.ctypes.data, net[1], int(net[2]), 0, l, C.addressof(at), C.addressof(k), C.addressof(padded))
        out.append(slice(int(at.value), int(at.value) + (int(k.value) + 1) * int(padded.value)))
    return out


def host_pack(sd, om_width=0):
    """The packed image of a state_dict by the header's own pack, in the wide build."""
    from ebcsim.sarl_train import LAYER_KEYS, shape_of
    net = shape_of(sd)
    w = [np.ascontiguousarray(sd[k + ".weight"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    b = [np.ascontiguousarray(sd[k + ".bias"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    P = np.full(host_floats(net, om_width), -7.0, dtype=np.float32)
    wp, bp, wd = (C.c_void_p * 11)(*[a.ctypes.data for a in w]), (C.c_void_p * 11)(*[a.ctypes.data for a in b]), _w(rotated(net, om_width))
    host_lib().sarl_grad_layers_host_pack(wd.ctypes.data, net[1], int(net[2]), int(om_width), wp, bp, P.ctypes.data)
    return P


def host_grad(P, net, rows, target, n_valid=None, mask=None, grad_scale=1.0, om_width=0):
    """(grad, loss_sum, count, value [B], attention [B, R]) of the wide host build; net[0][0] is the rows' width."""
    widths, S, glob = net
    rows, target = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    B, R, T = rows.shape
    assert T == widths[0] and target.shape == (B,)
    P = np.ascontiguousarray(P, dtype=np.float32)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    grad = np.full(P.shape, -7.0, dtype=np.float32)
    loss, count = C.c_double(-1.0), C.c_longlong(-1)
    value, att, wd = np.full((B,), -7.0, dtype=np.float32), np.full((B, R), -7.0, dtype=np.float32), _w(rotated(net, om_width))
    host_lib().sarl_grad_layers_host(wd.ctypes.data, S, int(glob), int(om_width), P.ctypes.data, B, R, rows.ctypes.data,
                                     None if nv is None else nv.ctypes.data, target.ctypes.data, None if mk is None else mk.ctypes.data,
                                     float(grad_scale), grad.ctypes.data, C.addressof(loss), C.addressof(count), value.ctypes.data, att.ctypes.data)
    return grad, float(loss.value), int(count.value), value, att


def write_batches(path, batch_list):
    """The input file of the host program: batches of (net, P, rows, target, n_valid or None, mask or None, grad_scale), om_width 0."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batch_list)))
        for (widths, S, glob), P, rows, target, nv, mk, scale in batch_list:
            B, R, _ = rows.shape
            f.write(struct.pack("<19if", *widths, S, int(glob), B, R, int(nv is not None), int(mk is not None), 0, float(scale)))
            f.write(np.ascontiguousarray(P, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(target, dtype="<f4").tobytes())
            if mk is not None:
                f.write(np.ascontiguousarray(mk, dtype="u1").tobytes())


# ---------------------------------------------------------------------------------------------------------------- accuracy
_refs, _rows = {}, {}


def reference_of(net, B, R, seed):
    """sarl_grad_cases.reference_of for a network given by its shape (there: by its index into NETS)."""
    sd = base.random_state_dict(net)
    rows, target = base.plain_batch(net, B, R, seed=640000 + 10007 * seed + net[0][1] + 10 * B + R)
    s64, den64, _, _ = base.torch_scores(sd, rows, None, torch.float64)
    live, scale = np.ones(B, dtype=bool), 2.0 / B
    g64, l64, _ = base.torch_grad(sd, rows, target, None, live, scale, torch.float64)
    g32, l32, _ = base.torch_grad(sd, rows, target, None, live, scale, torch.float32)
    slices = layer_slices(net)
    err32 = {l: float(np.abs(g32[slices[l]] - g64[slices[l]]).max() / np.abs(g64[slices[l]]).max()) for l in base.compared_layers(R)}
    return dict(net=net, sd=sd, rows=rows, target=target, scale=scale, g64=g64, l64=l64, err32=err32, loss32=abs(l32 - l64) / l64,
                min_abs_score=float(np.abs(s64).min()), min_den=float(den64.min()), slices=slices)


def chosen_reference(net, B, R):
    """reference_of the first seed (0, 1, ...) that sarl_grad_cases.usable takes."""
    key = (tuple(net[0]), B, R)
    if key not in _refs:
        for seed in range(base.MAX_SEEDS):
            ref = reference_of(net, B, R, seed)
            if base.usable(ref):
                ref["seed"] = seed
                _refs[key] = ref
                break
        else:
            raise AssertionError("no usable seed below %d for %s, B %d, R %d" % (base.MAX_SEEDS, net[0], B, R))
    return _refs[key]


def accuracy_row(net, B, R):
    """sarl_grad_cases.accuracy_row on the wide host build: per compared layer (name, err_rule, err_torch32), the loss's
    pair, and the seed; computed once."""
    key = (tuple(net[0]), B, R)
    if key not in _rows:
        from ebcsim.sarl_train import LAYER_KEYS
        ref = chosen_reference(net, B, R)
        g, loss, count, _, _ = host_grad(host_pack(ref["sd"]), net, ref["rows"], ref["target"], grad_scale=ref["scale"])
        assert count == B
        g64, sl = ref["g64"], ref["slices"]
        layers = [(LAYER_KEYS[l], float(np.abs(g[sl[l]].astype(np.float64) - g64[sl[l]]).max() / np.abs(g64[sl[l]]).max()), ref["err32"][l])
                  for l in base.compared_layers(R)]
        _rows[key] = (layers, (abs(loss - ref["l64"]) / ref["l64"], ref["loss32"]), ref["seed"])
    return _rows[key]


def accuracy_table():
    lines = ["SARL gradient rule (csrc/ebc_sarl_grad_rule.h, the wide host build tests/native/sarl_grad_layers_host.cc) at the widths of the",
             "layer form, against torch autograd of SarlModule in float64, beside torch's own float32 autograd:",
             "err = max |g - g_64| / max |g_64| per layer (W and bias together).  Bar: rule <= %d x torch32.  Seeds as in" % TOL_FACTOR,
             "profiles/sarl_grad_accuracy.txt (tests/sarl_grad_cases.py: usable).", "",
             "%-4s %4s %3s  %-16s %11s %11s %7s" % ("net", "B", "R", "layer", "err_rule", "err_torch32", "ratio")]
    for name, net in (("x2", X2_NET), ("x4", X4_NET)):
        lines.insert(-1, "%s: %s" % (name, base.net_name(net)))
    ratio = lambda a, b: a / b if b else (float("inf") if a else 0.0)  # noqa: E731
    for name, net, B, R in ACCURACY_CASES:
        layers, (lr, lt), _ = accuracy_row(net, B, R)
        for key, er, et in layers:
            lines.append("%-4s %4d %3d  %-16s %11.3e %11.3e %7.2f" % (name, B, R, key, er, et, ratio(er, et)))
        lines.append("%-4s %4d %3d  %-16s %11.3e %11.3e %7.2f" % (name, B, R, "loss_sum", lr, lt, ratio(lr, lt)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "sarl_grad_layers_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
