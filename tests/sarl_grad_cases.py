"""Shared by tests/test_sarl_train_cpu.py and tests/test_sarl_train_gpu.py: the host build of the SARL gradient rule
(tests/native/sarl_grad_host.cc: the source the kernel compiles, built with g++), seeded networks and batches, torch's
autograd of SarlModule as the reference, the edge batches, and the accuracy table both the test and
profiles/sarl_grad_accuracy.txt come from.

Bar.  The yardstick is the project's (tests/cadrl_cases.py, tests/sail_cases.py): torch's own float32 autograd against the
same computation in float64 on the same float32 weights and inputs.  Per layer (its W and bias together)
err = max |g - g_64| / max |g_64|; the rule's error must stay within TOL_FACTOR (8) times torch's float32 error.  Both are
float32 evaluations of the same sums: serial fmaf chains against torch's blocked sums.  The softmax needed no other
factor (profiles/sarl_grad_accuracy.txt).

Preconditions of a seed, none of which looks at the rule's result: in float64 no score is exactly 0 and no softmax
denominator is 0 (the reference's e = exp(s) * (s != 0) is discontinuous there); torch's float32 error is a yardstick at
all (`usable`: at least 2^-25 per layer, what rounding to float32 costs).  Per case the first seed that meets them is taken.
With R = 1 the softmax weight is 1 whatever the score: the attention stack's exact gradient is 0, there is nothing to take
a relative error of, and those three layers are left to test_one_row_gives_weight_one (where the rule's are exactly 0)."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

from cadrl_cases import TOL_FACTOR  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "sarl_grad_host.cc")
# the row width, then the units of mlp1 (2), mlp2 (2), attention (3), mlp3 (4)
REFERENCE_WIDTHS = [13, 150, 100, 100, 50, 100, 100, 1, 150, 100, 100, 1]
NARROW_WIDTHS = [13, 33, 18, 17, 6, 9, 7, 1, 11, 5, 3, 1]
NARROW_WIDE_ROWS = [17] + NARROW_WIDTHS[1:]
# (widths, self_state_dim, with_global_state)
REFERENCE_NET = (REFERENCE_WIDTHS, 6, True)
NARROW_NET = (NARROW_WIDTHS, 6, True)
NARROW_T17_NET = (NARROW_WIDE_ROWS, 6, True)
NARROW_LOCAL_NET = (NARROW_WIDTHS, 6, False)
NETS = [REFERENCE_NET, NARROW_NET, NARROW_T17_NET, NARROW_LOCAL_NET]
BATCHES = [1, 3, 4, 5, 9]  # 1, C - 1, C, C + 1, 2 C + 1 at the chunk size C = 4 (batches() checks it against the header)
ROWS = [1, 2, 5, 10]
EDGE_KINDS = ["plain", "ragged", "no_rows", "negative_rows", "rows_above", "masked", "nan_masked", "nan_padding"]
ATTENTION_LAYERS = (4, 5, 6)

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/sarl_grad_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="sarl_grad_host_")
        L = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libsarl_grad_host.so")))
        L.sarl_grad_host_chunk.restype = C.c_int
        L.sarl_grad_host_max_chunks.restype = C.c_int
        L.sarl_grad_host_refused.restype, L.sarl_grad_host_refused.argtypes = C.c_int, [C.c_void_p, C.c_int]
        L.sarl_grad_host_floats.restype, L.sarl_grad_host_floats.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.c_int]
        L.sarl_grad_host_layer.restype, L.sarl_grad_host_layer.argtypes = None, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.sarl_grad_host_pack.restype, L.sarl_grad_host_pack.argtypes = None, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.sarl_grad_host.restype = None
        L.sarl_grad_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 5
        _host["lib"] = L
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="sarl_grad_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "sarl_grad_host"))
    return _host[key]


def _w(widths):
    return np.ascontiguousarray(widths, dtype=np.int32)


def chunk():
    """EBC_SARL_GRAD_CHUNK, from the header itself."""
    return int(host_lib().sarl_grad_host_chunk())


def max_chunks():
    """EBC_SARL_GRAD_MAX_CHUNKS, the chunks one launch of the kernel takes, from the header itself."""
    return int(host_lib().sarl_grad_host_max_chunks())


def batches():
    c = chunk()
    assert BATCHES == [1, c - 1, c, c + 1, 2 * c + 1]
    return BATCHES


def host_floats(net):
    widths, S, glob = net
    w = _w(widths)
    return int(host_lib().sarl_grad_host_floats(w.ctypes.data, S, int(glob)))


def host_layers(net):
    """[(offset of W, inputs, padded units)] per layer, from the header itself."""
    widths, S, glob = net
    w, out = _w(widths), []
    for l in range(11):
        at, k, padded = C.c_longlong(-1), C.c_int(-1), C.c_int(-1)
        host_lib().sarl_grad_host_layer(w.ctypes.data, S, int(glob), l, C.addressof(at), C.addressof(k), C.addressof(padded))
        out.append((int(at.value), int(k.value), int(padded.value)))
    return out


def layer_slices(net):
    return [slice(at, at + (k + 1) * op) for at, k, op in host_layers(net)]


def module(net, dtype=torch.float32):
    from ebcsim.train import SarlModule
    w, S, glob = net
    return SarlModule(w[0], list(w[1:3]), list(w[3:5]), list(w[8:12]), list(w[5:8]), with_global_state=glob, self_state_dim=S).to(dtype)


def random_state_dict(net, seed=3):
    """A seeded SarlModule's state_dict (torch's default initialisation), float32 on the CPU."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 * seed + net[0][1] + net[0][0] + 7 * int(net[2]))
        m = module(net)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def host_pack(sd):
    """The packed image of a state_dict by the header's own pack (float32 [packed floats])."""
    from ebcsim.sarl_train import LAYER_KEYS, shape_of
    net = shape_of(sd)
    w = [np.ascontiguousarray(sd[k + ".weight"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    b = [np.ascontiguousarray(sd[k + ".bias"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    P = np.full(host_floats(net), -7.0, dtype=np.float32)
    wp, bp, wd = (C.c_void_p * 11)(*[a.ctypes.data for a in w]), (C.c_void_p * 11)(*[a.ctypes.data for a in b]), _w(net[0])
    host_lib().sarl_grad_host_pack(wd.ctypes.data, net[1], int(net[2]), wp, bp, P.ctypes.data)
    return P


def host_grad(P, net, rows, target, n_valid=None, mask=None, grad_scale=1.0):
    """(grad float32 [packed floats], loss_sum, count, value [B] float32, attention [B, R] float32) of the host build."""
    widths, S, glob = net
    rows, target = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    B, R, T = rows.shape
    assert T == widths[0] and target.shape == (B,)
    P = np.ascontiguousarray(P, dtype=np.float32)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    grad = np.full(P.shape, -7.0, dtype=np.float32)
    loss, count = C.c_double(-1.0), C.c_longlong(-1)
    value, att, wd = np.full((B,), -7.0, dtype=np.float32), np.full((B, R), -7.0, dtype=np.float32), _w(widths)
    host_lib().sarl_grad_host(wd.ctypes.data, S, int(glob), P.ctypes.data, B, R, rows.ctypes.data, None if nv is None else nv.ctypes.data,
                              target.ctypes.data, None if mk is None else mk.ctypes.data, float(grad_scale), grad.ctypes.data,
                              C.addressof(loss), C.addressof(count), value.ctypes.data, att.ctypes.data)
    return grad, float(loss.value), int(count.value), value, att


def write_batches(path, batch_list):
    """The input file of the host program (the format is in sarl_grad_host.cc): batches of (net, P, rows, target,
    n_valid or None, mask or None, grad_scale)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batch_list)))
        for (widths, S, glob), P, rows, target, nv, mk, scale in batch_list:
            B, R, _ = rows.shape
            f.write(struct.pack("<18if", *widths, S, int(glob), B, R, int(nv is not None), int(mk is not None), float(scale)))
            f.write(np.ascontiguousarray(P, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(target, dtype="<f4").tobytes())
            if mk is not None:
                f.write(np.ascontiguousarray(mk, dtype="u1").tobytes())


def read_results(path, batch_list):
    raw, at, out = open(path, "rb").read(), 0, []
    for _, P, rows, _, _, _, _ in batch_list:
        (B, R, _), n = rows.shape, len(P)
        grad = np.frombuffer(raw, "<f4", n, at)
        at += 4 * n
        loss, count = struct.unpack_from("<dq", raw, at)
        at += 16
        value = np.frombuffer(raw, "<f4", B, at)
        at += 4 * B
        out.append((grad, loss, count, value, np.frombuffer(raw, "<f4", B * R, at).reshape(B, R)))
        at += 4 * B * R
    assert at == len(raw)
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plain_batch(net, B, R, seed=None):
    """Ordinary states: (rows [B, R, T] float32, target [B] float32), rows like rotated joint states in size."""
    widths = net[0]
    rs = np.random.RandomState(620000 + 1000 * widths[1] + 10 * B + R if seed is None else seed)
    return rs.normal(0.0, 1.0, (B, R, widths[0])).astype(np.float32), rs.normal(0.0, 0.5, (B,)).astype(np.float32)


def edge_batch(net, B, R, seed=None):
    """plain_batch with a state of every kind of EDGE_KINDS in turn (state b has kind (b + R) % 8, so the shapes together
    cover them all at B = 1): (rows, target, n_valid [B] int64, mask [B] uint8, kinds [B]).
      ragged         1 <= n_valid < R        no_rows: n_valid 0        negative_rows: n_valid -3        rows_above: n_valid R + 5
      masked         mask 0, ordinary values        nan_masked: mask 0, NaN and infinities in its rows and its target
      nan_padding    n_valid < R and NaN, +inf, -inf in the rows past it
    Rows at or past n_valid of every state hold NaN, +inf and -inf in turn."""
    rows, target = plain_batch(net, B, R, seed)
    rs = np.random.RandomState((7 if seed is None else seed) + 13 * B + R)
    nv, mask, kinds = np.full((B,), R, dtype=np.int64), np.ones((B,), dtype=np.uint8), []
    for b in range(B):
        kind = EDGE_KINDS[(b + R) % len(EDGE_KINDS)]
        kinds.append(kind)
        if kind in ("ragged", "nan_padding"):
            nv[b] = rs.randint(1, R) if R > 1 else 1
        elif kind == "no_rows":
            nv[b] = 0
        elif kind == "negative_rows":
            nv[b] = -3
        elif kind == "rows_above":
            nv[b] = R + 5
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


def module_forward(m, x, nv, dtype):
    """SarlModule's forward (SarlValueNet's torch body on the module's parameters) in `dtype`: the network view computes in
    float32 and returns float32 values by default, so its dtype is set and mlp3 is applied without the cast back."""
    from ebcsim.sarl import _mlp
    vn = m.as_value_net()
    vn.dtype = dtype
    vn._value = lambda rows, attended, nat, f32=False: _mlp(
        torch.cat([rows[:, 0, :vn.self_state_dim], attended], dim=1), vn.mlp3, False).squeeze(1)
    return vn._forward(x, nv)


def torch_grad(sd, rows, target, n_valid, live, grad_scale, dtype):
    """torch autograd of SarlModule in `dtype` on the float32 weights and the live states' float32 inputs (rows past
    n_valid zeroed: autograd multiplies them with zero weights): (packed gradient as a float64 array, loss_sum, value
    [live]) of grad_scale / 2 * the sum of squared differences."""
    from ebcsim.sarl_train import pack_state_dict, shape_of
    from ebcsim.train import SarlModule
    net = shape_of(sd)
    m = module(net, dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    idx, x, nv = _live_inputs(rows, n_valid, live)
    v = module_forward(m, torch.from_numpy(x).to(dtype), nv, dtype)
    d = v - torch.from_numpy(np.asarray(target, dtype=np.float32)[idx]).to(dtype)
    loss = (d * d).sum()
    (0.5 * float(grad_scale) * loss).backward()
    g = pack_state_dict({SarlModule._ref_name(k): p.grad.to(torch.float64) for k, p in m.named_parameters()},
                        out=torch.zeros(host_floats(net), dtype=torch.float64))
    return g.numpy(), float(loss.detach()), v.detach().double().numpy()


def torch_scores(sd, rows, n_valid, dtype):
    """(scores [B, R], softmax denominators [B], weights [B, R], values [B]) of the network in `dtype`, written out in plain
    torch from rl/policy/sarl.py:38-82 on the rows < n_valid; as float64 arrays."""
    net = shape_of_sd(sd)
    S, glob = net[1], net[2]
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = torch.from_numpy(np.asarray(rows, dtype=np.float32)).to(dtype)
    B, R, T = x.shape
    nv = torch.full((B,), R, dtype=torch.int64) if n_valid is None else torch.from_numpy(np.clip(np.asarray(n_valid), 0, R))
    valid = torch.arange(R)[None, :] < nv[:, None]
    x = torch.where(valid[:, :, None], x, torch.zeros_like(x))

    def mlp(v, name, idx, last_relu):
        for j, i in enumerate(idx):
            v = torch.nn.functional.linear(v, p["%s.%d.weight" % (name, i)], p["%s.%d.bias" % (name, i)])
            if j < len(idx) - 1 or last_relu:
                v = torch.relu(v)
        return v
    with torch.no_grad():
        h1 = mlp(x.reshape(B * R, T), "mlp1", (0, 2), True)
        ft = mlp(h1, "mlp2", (0, 2), False).view(B, R, -1)
        a_in = h1
        if glob:
            g = (h1.view(B, R, -1) * valid[:, :, None]).sum(1) / nv.clamp(min=1).to(dtype)[:, None]
            a_in = torch.cat([h1.view(B, R, -1), g[:, None, :].expand(B, R, g.shape[1])], dim=2).reshape(B * R, -1)
        s = mlp(a_in, "attention", (0, 2, 4), False).view(B, R)
        e = torch.exp(s) * (s != 0).to(dtype) * valid
        den = e.sum(1)
        w = e / den[:, None]
        joint = torch.cat([x[:, 0, :S], (w[:, :, None] * ft).sum(1)], dim=1)
        v = mlp(joint, "mlp3", (0, 2, 4, 6), False).squeeze(1)
    return s.double().numpy(), den.double().numpy(), w.double().numpy(), v.double().numpy()


def shape_of_sd(sd):
    from ebcsim.sarl_train import shape_of
    return shape_of(sd)


def accuracy_cases():
    return [(ni, B, R) for ni in (0, 1) for B in batches() for R in (1, 5)] + [(0, 100, 5), (0, 100, 10), (3, 2 * chunk() + 1, 5)]


_rows = {}
YARDSTICK_FLOOR = 2.0 ** -25
MAX_SEEDS = 2000


def compared_layers(R):
    return [l for l in range(11) if not (R == 1 and l in ATTENTION_LAYERS)]


def reference_of(ni, B, R, seed):
    """What the comparison of one seeded batch needs and the code under test has no part in: the batch, float64 and
    float32 autograd of SarlModule, torch's float32 error per layer and of the loss, the float64 scores and softmax
    denominators."""
    net = NETS[ni]
    sd = random_state_dict(net)
    rows, target = plain_batch(net, B, R, seed=630000 + 10007 * seed + 1000 * ni + 10 * B + R)
    s64, den64, _, _ = torch_scores(sd, rows, None, torch.float64)
    live, scale = np.ones(B, dtype=bool), 2.0 / B
    g64, l64, _ = torch_grad(sd, rows, target, None, live, scale, torch.float64)
    g32, l32, _ = torch_grad(sd, rows, target, None, live, scale, torch.float32)
    slices = layer_slices(net)
    err32 = {l: float(np.abs(g32[slices[l]] - g64[slices[l]]).max() / np.abs(g64[slices[l]]).max()) for l in compared_layers(R)}
    return dict(net=net, sd=sd, rows=rows, target=target, scale=scale, g64=g64, l64=l64, err32=err32, loss32=abs(l32 - l64) / l64,
                min_abs_score=float(np.abs(s64).min()), min_den=float(den64.min()), slices=slices)


def usable(ref):
    """The preconditions of a seed.  (1) In float64 no score is exactly 0 and no softmax denominator is 0.  (2) The
    yardstick is one: torch's float32 error of every compared layer and of the loss is at least 2^-25 of the layer's
    largest entry, which is what rounding the exact result to float32 costs on average; a draw in which torch's float32
    result happens to land closer than that to the float64 one measures luck, not float32 arithmetic.  Neither condition
    looks at the rule's result."""
    return (ref["min_abs_score"] > 0 and ref["min_den"] > 0 and min(ref["err32"].values()) >= YARDSTICK_FLOOR
            and ref["loss32"] >= YARDSTICK_FLOOR)


_refs = {}


def chosen_reference(ni, B, R):
    """reference_of the first seed (0, 1, ...) that is usable."""
    if (ni, B, R) not in _refs:
        for seed in range(MAX_SEEDS):
            ref = reference_of(ni, B, R, seed)
            if usable(ref):
                ref["seed"] = seed
                _refs[ni, B, R] = ref
                break
        else:
            raise AssertionError("no usable seed below %d for net %d, B %d, R %d" % (MAX_SEEDS, ni, B, R))
    return _refs[ni, B, R]


def accuracy_row(ni, B, R):
    """Per compared layer (name, err_rule, err_torch32), the loss's (err_rule, err_torch32), the precondition (smallest
    |score| and smallest softmax denominator in float64) and the seed, of the chosen seeded batch; computed once."""
    if (ni, B, R) not in _rows:
        from ebcsim.sarl_train import LAYER_KEYS
        ref = chosen_reference(ni, B, R)
        g, loss, count, value, att = host_grad(host_pack(ref["sd"]), ref["net"], ref["rows"], ref["target"], grad_scale=ref["scale"])
        assert count == B
        g64, sl = ref["g64"], ref["slices"]
        layers = [(LAYER_KEYS[l], float(np.abs(g[sl[l]].astype(np.float64) - g64[sl[l]]).max() / np.abs(g64[sl[l]]).max()), ref["err32"][l])
                  for l in compared_layers(R)]
        _rows[ni, B, R] = (layers, (abs(loss - ref["l64"]) / ref["l64"], ref["loss32"]), (ref["min_abs_score"], ref["min_den"]), ref["seed"])
    return _rows[ni, B, R]


def net_name(net):
    return "-".join(str(w) for w in net[0]) + ("" if net[2] else " (no global state)")


def accuracy_table():
    lines = ["SARL gradient rule (csrc/ebc_sarl_grad_rule.h, host build) against torch autograd of SarlModule in float64,",
             "beside torch's own float32 autograd: err = max |g - g_64| / max |g_64| per layer (W and bias together).",
             "EBC_SARL_GRAD_CHUNK = %d.  Seeded networks and inputs of tests/sarl_grad_cases.py; bar: rule <= %d x torch32."
             % (chunk(), TOL_FACTOR),
             "Per case the first seed with no float64 score of 0, no float64 softmax denominator of 0 and torch32 errors all at",
             "least 2^-25 (tests/sarl_grad_cases.py: usable).  R = 1 leaves out the attention layers (their exact gradient is 0).", "",
             "%-4s %4s %3s  %-16s %11s %11s %7s" % ("net", "B", "R", "layer", "err_rule", "err_torch32", "ratio")]
    ratio = lambda a, b: a / b if b else (float("inf") if a else 0.0)  # noqa: E731
    for i, net in enumerate(NETS):
        lines.insert(-1, "net %d: %s" % (i, net_name(net)))
    for ni, B, R in accuracy_cases():
        layers, (lr, lt), _, _ = accuracy_row(ni, B, R)
        for key, er, et in layers:
            lines.append("%-4d %4d %3d  %-16s %11.3e %11.3e %7.2f" % (ni, B, R, key, er, et, ratio(er, et)))
        lines.append("%-4d %4d %3d  %-16s %11.3e %11.3e %7.2f" % (ni, B, R, "loss_sum", lr, lt, ratio(lr, lt)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "sarl_grad_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
