"""Shared by tests/test_lstm_train_cpu.py and tests/test_lstm_train_gpu.py: the host build of the LSTM-RL gradient rule
(tests/native/lstm_grad_host.cc: the source the kernel compiles, built with g++), seeded networks and batches, the golden
LSTM runs' rows, torch's autograd of LstmModule as the reference, the edge batches, and the accuracy table both the test
and profiles/lstm_grad_accuracy.txt come from.

Bar.  The yardstick is the project's (tests/cadrl_cases.py, tests/sarl_grad_cases.py): torch's own float32 autograd against
the same computation in float64 on the same float32 weights and inputs.  Per parameter tensor err = max |g - g_64| /
max |g_64|; the rule's error must stay within TOL_FACTOR (8) times torch's float32 error.  Both are float32 evaluations of
the same sums: serial fmaf chains and the cell's own sigmoid / tanh (csrc/ebc_lstm_cell.h) against torch's blocked sums
and its libm.

Precondition of a seed, which does not look at the rule's result: torch's float32 error is a yardstick at all (`usable`:
at least 2^-25 per tensor and for the loss, what rounding to float32 costs).  Per case the first seed that meets it is
taken."""
import ctypes as C
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

from cadrl_cases import TOL_FACTOR  # noqa: F401
from helpers import load
from lstm_cases import RUNS, SCALES, golden_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "lstm_grad_host.cc")
# (widths, self_state_dim, with_interaction_module); widths: the row width, mlp1's four units (zeros without mlp1), H, mlp's four
REFERENCE_NET2 = ([13, 150, 100, 100, 50, 50, 150, 100, 100, 1], 6, True)
REFERENCE_NET1 = ([13, 0, 0, 0, 0, 50, 150, 100, 100, 1], 6, False)
NARROW_NET2 = ([13, 12, 8, 8, 6, 7, 10, 8, 8, 1], 6, True)  # H is no multiple of 4
NARROW_NET1 = ([13, 0, 0, 0, 0, 7, 10, 8, 8, 1], 6, False)
NETS = [REFERENCE_NET2, REFERENCE_NET1, NARROW_NET2, NARROW_NET1]
BATCHES = [1, 3, 4, 5, 9]  # 1, C - 1, C, C + 1, 2 C + 1 at the chunk size C = 4 (batches() checks it against the header)
ROWS = [1, 2, 5]
EDGE_KINDS = ["plain", "one_row", "no_rows", "negative_rows", "rows_above", "masked", "nan_masked", "ragged"]

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/lstm_grad_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="lstm_grad_host_")
        L = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "liblstm_grad_host.so")))
        L.lstm_grad_host_chunk.restype = C.c_int
        L.lstm_grad_host_max_chunks.restype = C.c_int
        L.lstm_grad_host_refused.restype, L.lstm_grad_host_refused.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]
        L.lstm_grad_host_floats.restype, L.lstm_grad_host_floats.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.c_int]
        L.lstm_grad_host_layer.restype, L.lstm_grad_host_layer.argtypes = None, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.lstm_grad_host_pack.restype, L.lstm_grad_host_pack.argtypes = None, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        L.lstm_grad_host.restype = None
        L.lstm_grad_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 5
        _host["lib"] = L
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="lstm_grad_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "lstm_grad_host"))
    return _host[key]


def _w(widths):
    return np.ascontiguousarray(widths, dtype=np.int32)


def chunk():
    """EBC_LSTM_GRAD_CHUNK, from the header itself."""
    return int(host_lib().lstm_grad_host_chunk())


def max_chunks():
    return int(host_lib().lstm_grad_host_max_chunks())


def batches():
    c = chunk()
    assert BATCHES == [1, c - 1, c, c + 1, 2 * c + 1]
    return BATCHES


def host_floats(net):
    widths, S, two = net
    return int(host_lib().lstm_grad_host_floats(_w(widths).ctypes.data, S, int(two)))


def host_layers(net):
    """[(offset, inputs, padded units)] of the eight Linear layers and, last, of the cell ((I + H + 2) rows of 4 H: its
    `inputs` is I + H + 1), from the header itself."""
    widths, S, two = net
    w, out = _w(widths), []
    for l in range(9):
        at, k, padded = C.c_longlong(-1), C.c_int(-1), C.c_int(-1)
        host_lib().lstm_grad_host_layer(w.ctypes.data, S, int(two), l, C.addressof(at), C.addressof(k), C.addressof(padded))
        out.append((int(at.value), int(k.value), int(padded.value)))
    return out


def module(net, dtype=torch.float32):
    from ebcsim.lstm_rl import LstmModule
    w, S, two = net
    return LstmModule(w[0], S, list(w[6:10]), w[5], list(w[1:5]) if two else None).to(dtype)


def random_state_dict(net, seed=3, scale=1.0):
    """A seeded LstmModule's state_dict (torch's default initialisation, the LSTM's four tensors times `scale`: 4 takes the
    gates out of their linear range, as lstm_cases.SCALES), float32 on the CPU."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 * seed + net[0][5] + net[0][1] + 7 * int(net[2]))
        m = module(net)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k in sd:
        if k.startswith("lstm."):
            sd[k] = sd[k] * float(scale)
    return sd


def net_of(sd):
    from ebcsim.lstm_train import shape_of
    return shape_of(sd)


def host_pack(sd):
    """The packed image of a state_dict by the header's own pack (float32 [packed floats])."""
    from ebcsim.lstm_train import LSTM_KEYS, MLP1_KEYS, MLP_KEYS
    net = net_of(sd)
    keys = (list(MLP1_KEYS) if net[2] else [None] * 4) + list(MLP_KEYS)
    w = [None if k is None else np.ascontiguousarray(sd[k + ".weight"].numpy(), dtype=np.float32) for k in keys]
    b = [None if k is None else np.ascontiguousarray(sd[k + ".bias"].numpy(), dtype=np.float32) for k in keys]
    cell = [np.ascontiguousarray(sd[k].numpy(), dtype=np.float32) for k in LSTM_KEYS]
    P = np.full(host_floats(net), -7.0, dtype=np.float32)
    wp = (C.c_void_p * 8)(*[None if a is None else a.ctypes.data for a in w])
    bp = (C.c_void_p * 8)(*[None if a is None else a.ctypes.data for a in b])
    host_lib().lstm_grad_host_pack(_w(net[0]).ctypes.data, net[1], int(net[2]), wp, bp, *[a.ctypes.data for a in cell], P.ctypes.data)
    return P


def host_grad(P, net, rows, target, n_valid=None, mask=None, grad_scale=1.0):
    """(grad float32 [packed floats], loss_sum, count, value [B] float32, joint [B, S + H] float32) of the host build."""
    widths, S, two = net
    rows, target = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    B, R, T = rows.shape
    assert T == widths[0] and target.shape == (B,)
    P = np.ascontiguousarray(P, dtype=np.float32)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    grad = np.full(P.shape, -7.0, dtype=np.float32)
    loss, count = C.c_double(-1.0), C.c_longlong(-1)
    value, joint, wd = np.full((B,), -7.0, dtype=np.float32), np.full((B, S + widths[5]), -7.0, dtype=np.float32), _w(widths)
    host_lib().lstm_grad_host(wd.ctypes.data, S, int(two), P.ctypes.data, B, R, rows.ctypes.data, None if nv is None else nv.ctypes.data,
                              target.ctypes.data, None if mk is None else mk.ctypes.data, float(grad_scale), grad.ctypes.data,
                              C.addressof(loss), C.addressof(count), value.ctypes.data, joint.ctypes.data)
    return grad, float(loss.value), int(count.value), value, joint


def write_batches(path, batch_list):
    """The input file of the host program (the format is in lstm_grad_host.cc): batches of (net, P, rows, target,
    n_valid or None, mask or None, grad_scale)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batch_list)))
        for (widths, S, two), P, rows, target, nv, mk, scale in batch_list:
            B, R, _ = rows.shape
            f.write(struct.pack("<16if", *widths, S, int(two), B, R, int(nv is not None), int(mk is not None), float(scale)))
            f.write(np.ascontiguousarray(P, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(target, dtype="<f4").tobytes())
            if mk is not None:
                f.write(np.ascontiguousarray(mk, dtype="u1").tobytes())


def read_results(path, batch_list):
    raw, at, out = open(path, "rb").read(), 0, []
    for (widths, S, _), P, rows, _, _, _, _ in batch_list:
        B, n, J = rows.shape[0], len(P), S + widths[5]
        grad = np.frombuffer(raw, "<f4", n, at)
        at += 4 * n
        loss, count = struct.unpack_from("<dq", raw, at)
        at += 16
        value = np.frombuffer(raw, "<f4", B, at)
        at += 4 * B
        out.append((grad, loss, count, value, np.frombuffer(raw, "<f4", B * J, at).reshape(B, J)))
        at += 4 * B * J
    assert at == len(raw)
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plain_batch(net, B, R, seed=None):
    """Ordinary states: (rows [B, R, T] float32, target [B] float32), rows like rotated joint states in size."""
    widths = net[0]
    rs = np.random.RandomState(720000 + 1000 * widths[5] + 100 * int(net[2]) + 10 * B + R if seed is None else seed)
    return rs.normal(0.0, 1.0, (B, R, widths[0])).astype(np.float32), rs.normal(0.0, 0.5, (B,)).astype(np.float32)


def edge_batch(net, B, R, seed=None):
    """plain_batch with a state of every kind of EDGE_KINDS in turn (state b has kind (b + R) % 8, so the shapes together
    cover them all at B = 1): (rows, target, n_valid [B] int64, mask [B] uint8, kinds [B]).
      one_row        n_valid 1        no_rows: n_valid 0        negative_rows: n_valid -1        rows_above: n_valid R + 3
      masked         mask 0, ordinary values        nan_masked: mask 0, NaN and infinities in its rows and its target
      ragged         1 <= n_valid <= R, drawn        plain: n_valid R
    Rows at or past n_valid of every state (the padding rows) hold NaN, +inf and -inf in turn."""
    rows, target = plain_batch(net, B, R, seed)
    rs = np.random.RandomState((7 if seed is None else seed) + 13 * B + R)
    nv, mask, kinds = np.full((B,), R, dtype=np.int64), np.ones((B,), dtype=np.uint8), []
    for b in range(B):
        kind = EDGE_KINDS[(b + R) % len(EDGE_KINDS)]
        kinds.append(kind)
        if kind == "ragged":
            nv[b] = rs.randint(1, R + 1)
        elif kind == "one_row":
            nv[b] = 1
        elif kind == "no_rows":
            nv[b] = 0
        elif kind == "negative_rows":
            nv[b] = -1
        elif kind == "rows_above":
            nv[b] = R + 3
        elif kind == "masked":
            mask[b] = 0
        elif kind == "nan_masked":
            mask[b] = 0
            rows[b, rs.randint(R), rs.randint(net[0][0])] = np.nan
            rows[b, rs.randint(R), 0] = np.inf
            target[b] = np.nan
        for r in range(max(0, min(R, int(nv[b]))), R):
            rows[b, r] = (np.nan, np.inf, -np.inf)[(r + b) % 3]
    return rows, target, nv, mask, kinds


def is_live(nv, mask):
    return (np.asarray(nv) >= 1) & (np.asarray(mask) != 0)


def _live_inputs(rows, n_valid, live):
    idx = np.nonzero(live)[0]
    x = np.array(np.asarray(rows)[idx], dtype=np.float32)
    R = x.shape[1]
    nv = None
    if n_valid is not None:
        nv = np.clip(np.asarray(n_valid)[idx], 0, R)
        x[np.arange(R)[None, :] >= nv[:, None]] = 0.0
        nv = torch.from_numpy(nv)
    return idx, x, nv


def torch_grad(sd, rows, target, n_valid, live, grad_scale, dtype):
    """torch autograd of LstmModule in `dtype` on the float32 weights and the live states' float32 inputs (rows past
    n_valid zeroed: they never reach h_n, autograd multiplies them with zero deltas): ({key: gradient as a float64 array},
    loss_sum, value [live]) of grad_scale / 2 * the sum of squared differences."""
    m = module(net_of(sd), dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    idx, x, nv = _live_inputs(rows, n_valid, live)
    v = m(torch.from_numpy(x).to(dtype), nv).squeeze(1)
    d = v - torch.from_numpy(np.asarray(target, dtype=np.float32)[idx]).to(dtype)
    loss = (d * d).sum()
    (0.5 * float(grad_scale) * loss).backward()
    return {k: p.grad.double().numpy() for k, p in m.named_parameters()}, float(loss.detach()), v.detach().double().numpy()


def unpacked(net, g):
    """{key: float64 array in torch's shape} of a packed gradient."""
    from ebcsim.lstm_train import _views
    return {k: v.double().numpy() for k, v in _views(torch.from_numpy(np.ascontiguousarray(g)), *net).items()}


_golden = {}


def golden_rows(name):
    """(state_dict, rows [N, R, 13] float32, targets [N] float32) of a golden LSTM run: its network, the states its policy
    saw (last_state) and, as value targets, the values the reference recorded for the actions it chose."""
    if name not in _golden:
        z = load(name)
        meta = json.loads(str(z["meta"]))
        idx = [int(np.where((z["action_space"] == z["action"][t]).all(1))[0][0]) for t in range(len(z["action"]))]
        _golden[name] = (golden_state_dict(meta), np.ascontiguousarray(z["last_state"], dtype=np.float32),
                         np.array([z["values"][t, i] for t, i in enumerate(idx)], dtype=np.float32))
    return _golden[name]


def accuracy_cases():
    """("golden", run) and ("seeded", net index, B, R, gate scale)."""
    c = chunk()
    return [("golden", name) for name in RUNS] + [("seeded", ni, B, R, s) for ni in (2, 3) for (B, R) in ((2 * c + 1, 5), (c - 1, 2)) for s in SCALES] + [
        ("seeded", ni, 100, 10, s) for ni in (0, 1) for s in SCALES]


YARDSTICK_FLOOR = 2.0 ** -25
MAX_SEEDS = 200
_refs, _rows = {}, {}


def _err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def reference_of(case, seed):
    """What the comparison of one batch needs and the code under test has no part in: the batch, float64 and float32
    autograd of LstmModule, torch's float32 error per tensor and of the loss."""
    if case[0] == "golden":
        sd, rows, target = golden_rows(case[1])
    else:
        _, ni, B, R, s = case
        sd = random_state_dict(NETS[ni], seed=3 + seed, scale=s)
        rows, target = plain_batch(NETS[ni], B, R, seed=730000 + 10007 * seed + 1000 * ni + 10 * B + R)
    B = rows.shape[0]
    live, scale = np.ones(B, dtype=bool), 2.0 / B
    g64, l64, _ = torch_grad(sd, rows, target, None, live, scale, torch.float64)
    g32, l32, _ = torch_grad(sd, rows, target, None, live, scale, torch.float32)
    return dict(net=net_of(sd), sd=sd, rows=rows, target=target, scale=scale, g64=g64, l64=l64, err32={k: _err(g32[k], g64[k]) for k in g64},
                loss32=abs(l32 - l64) / l64)


def usable(ref):
    """The yardstick is one: torch's float32 error of every tensor and of the loss is at least 2^-25 of the tensor's
    largest entry, what rounding the exact result to float32 costs on average.  It does not look at the rule's result."""
    return min(ref["err32"].values()) >= YARDSTICK_FLOOR and ref["loss32"] >= YARDSTICK_FLOOR


def chosen_reference(case):
    """reference_of the first seed (0, 1, ...) that is usable; a golden run has one batch and is taken as it is."""
    if case not in _refs:
        for seed in range(1 if case[0] == "golden" else MAX_SEEDS):
            ref = reference_of(case, seed)
            if usable(ref) or case[0] == "golden":
                ref["seed"] = seed
                _refs[case] = ref
                break
        else:
            raise AssertionError("no usable seed below %d for %s" % (MAX_SEEDS, (case,)))
    return _refs[case]


def accuracy_row(case):
    """([(tensor, err_rule, err_torch32)], the loss's (err_rule, err_torch32), the seed) of the case; computed once."""
    if case not in _rows:
        ref = chosen_reference(case)
        g, loss, count, _, _ = host_grad(host_pack(ref["sd"]), ref["net"], ref["rows"], ref["target"], grad_scale=ref["scale"])
        assert count == ref["rows"].shape[0]
        got = unpacked(ref["net"], g)
        _rows[case] = ([(k, _err(got[k], ref["g64"][k]), ref["err32"][k]) for k in ref["g64"]],
                       (abs(loss - ref["l64"]) / ref["l64"], ref["loss32"]), ref["seed"])
    return _rows[case]


def case_name(case):
    if case[0] == "golden":
        return case[1]
    return "net %d B %d R %d scale %g" % case[1:]


def accuracy_table():
    lines = ["LSTM-RL gradient rule (csrc/ebc_lstm_grad_rule.h, host build) against torch autograd of LstmModule in float64,",
             "beside torch's own float32 autograd: err = max |g - g_64| / max |g_64| per parameter tensor.",
             "EBC_LSTM_GRAD_CHUNK = %d.  The golden LSTM runs' states with their recorded values as targets, and seeded networks and" % chunk(),
             "inputs of tests/lstm_grad_cases.py at gate scales 1 and 4; bar: rule <= %d x torch32.  Per seeded case the first seed" % TOL_FACTOR,
             "with torch32 errors all at least 2^-25 (tests/lstm_grad_cases.py: usable).  A golden run is one batch and is taken as",
             "it is: where torch's error of a tensor is below 2^-25 (3.0e-8, half a unit of float32's last place: no float32 result",
             "can be held to a multiple of less), the bar is %d x 2^-25 and the ratio printed here is against torch's error all the" % TOL_FACTOR,
             "same: lstm_interaction_n10's mlp.6.bias, ONE number, torch 2.0e-9, the rule 8.9e-8 (one and a half units), ratio 44.8."]
    for i, net in enumerate(NETS):
        lines.append("net %d: %s%s" % (i, "-".join(str(w) for w in net[0]), "" if net[2] else " (no mlp1)"))
    lines += ["", "%-34s %-22s %11s %11s %7s" % ("case", "tensor", "err_rule", "err_torch32", "ratio")]
    ratio = lambda a, b: a / b if b else (float("inf") if a else 0.0)  # noqa: E731
    for case in accuracy_cases():
        tensors, (lr, lt), _ = accuracy_row(case)
        for key, er, et in tensors:
            lines.append("%-34s %-22s %11.3e %11.3e %7.2f" % (case_name(case), key, er, et, ratio(er, et)))
        lines.append("%-34s %-22s %11.3e %11.3e %7.2f" % (case_name(case), "loss_sum", lr, lt, ratio(lr, lt)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "lstm_grad_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
