"""Shared by tests/test_cadrl_train_cpu.py and tests/test_cadrl_train_gpu.py: the host build of the CADRL gradient rule
(tests/native/cadrl_grad_host.cc: the source the kernel compiles, built with g++), seeded networks and batches, torch's
autograd of CadrlModule as the reference, the edge batches, and the accuracy table both the test and
profiles/cadrl_grad_accuracy.txt come from.

Bar.  The yardstick is the project's for the CADRL forward (tests/cadrl_cases.py): torch's own float32 autograd against
the same computation in float64 on the same float32 weights and inputs.  Per layer (its W and bias together)
err = max |g - g_64| / max |g_64|; the rule's error must stay within TOL_FACTOR (8, tests/cadrl_cases.py) times torch's
float32 error.  Both are float32 evaluations of the same sums: serial fmaf chains against torch's blocked sums.

A state's gradient goes through its minimal row, so the comparison needs the float32 forms and the float64 form to pick
the same row: the seeds below are chosen so that every state's float64 top-2 gap between its two smallest rows exceeds
twice the tolerance the VALUES are held to (TOL_FACTOR x torch's float32 forward error on the same rows), and the test
asserts it for every state: none is left out.  A seed must also make torch's float32 error a yardstick at all (`usable`:
at least 2^-25 per layer, what rounding to float32 costs); per case the first seed that meets both is taken, and neither
condition looks at the rule's result."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

from cadrl_cases import TOL_FACTOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "cadrl_grad_host.cc")
REFERENCE_WIDTHS = [13, 150, 100, 100, 1]
NARROW_WIDTHS = [13, 33, 17, 5, 1]
WIDTHS = [REFERENCE_WIDTHS, NARROW_WIDTHS]
BATCHES = [1, 15, 16, 17, 33]
ROWS = [1, 2, 5, 18]
EDGE_KINDS = ["plain", "tie", "ragged", "no_rows", "negative_rows", "rows_above", "masked", "nan_masked", "nan_padding"]

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/cadrl_grad_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="cadrl_grad_host_")
        L = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libcadrl_grad_host.so")))
        L.cadrl_grad_host_chunk.restype = C.c_int
        L.cadrl_grad_host_refused.restype, L.cadrl_grad_host_refused.argtypes = C.c_int, [C.c_void_p]
        L.cadrl_grad_host_floats.restype, L.cadrl_grad_host_floats.argtypes = C.c_longlong, [C.c_void_p]
        L.cadrl_grad_host_layer.restype, L.cadrl_grad_host_layer.argtypes = None, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.cadrl_grad_host_pack.restype, L.cadrl_grad_host_pack.argtypes = None, [C.c_void_p] * 4
        L.cadrl_grad_host.restype = None
        L.cadrl_grad_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 5
        _host["lib"] = L
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="cadrl_grad_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "cadrl_grad_host"))
    return _host[key]


def _w(widths):
    return np.ascontiguousarray(widths, dtype=np.int32)


def chunk():
    """EBC_CADRL_GRAD_CHUNK, from the header itself."""
    return int(host_lib().cadrl_grad_host_chunk())


def host_floats(widths):
    w = _w(widths)
    return int(host_lib().cadrl_grad_host_floats(w.ctypes.data))


def host_layers(widths):
    """[(offset of W, padded units)] per layer, from the header itself."""
    w, out = _w(widths), []
    for l in range(4):
        at, padded = C.c_longlong(-1), C.c_int(-1)
        host_lib().cadrl_grad_host_layer(w.ctypes.data, l, C.addressof(at), C.addressof(padded))
        out.append((int(at.value), int(padded.value)))
    return out


def layer_slices(widths):
    return [slice(at, at + (k + 1) * op) for (at, op), k in zip(host_layers(widths), widths[:-1])]


def random_state_dict(widths, seed=3):
    """A seeded CadrlModule's state_dict (torch's default initialisation), float32 on the CPU."""
    from ebcsim.cadrl import CadrlModule
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 * seed + widths[1])
        m = CadrlModule(widths[0], list(widths[1:]))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def host_pack(sd):
    """The packed image of a state_dict by the header's own pack (float32 [packed floats])."""
    from ebcsim.cadrl_train import LAYER_KEYS, widths_of
    widths = widths_of(sd)
    w = [np.ascontiguousarray(sd[k + ".weight"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    b = [np.ascontiguousarray(sd[k + ".bias"].numpy(), dtype=np.float32) for k in LAYER_KEYS]
    P = np.full(host_floats(widths), -7.0, dtype=np.float32)
    wp, bp, wd = (C.c_void_p * 4)(*[a.ctypes.data for a in w]), (C.c_void_p * 4)(*[a.ctypes.data for a in b]), _w(widths)
    host_lib().cadrl_grad_host_pack(wd.ctypes.data, wp, bp, P.ctypes.data)
    return P


def host_grad(P, widths, rows, target, n_valid=None, mask=None, grad_scale=1.0):
    """(grad float32 [packed floats], loss_sum, count, value [B] float32, min_row [B] int32) of the host build."""
    rows, target = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    B, R, T = rows.shape
    assert T == widths[0] and target.shape == (B,)
    P = np.ascontiguousarray(P, dtype=np.float32)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    grad = np.full(P.shape, -7.0, dtype=np.float32)
    loss, count = C.c_double(-1.0), C.c_longlong(-1)
    value, min_row, wd = np.full((B,), -7.0, dtype=np.float32), np.full((B,), -7, dtype=np.int32), _w(widths)
    host_lib().cadrl_grad_host(wd.ctypes.data, P.ctypes.data, B, R, rows.ctypes.data, None if nv is None else nv.ctypes.data,
                               target.ctypes.data, None if mk is None else mk.ctypes.data, float(grad_scale), grad.ctypes.data,
                               C.addressof(loss), C.addressof(count), value.ctypes.data, min_row.ctypes.data)
    return grad, float(loss.value), int(count.value), value, min_row


def write_batches(path, batches):
    """The input file of the host program (the format is in cadrl_grad_host.cc): batches of (widths, P, rows, target,
    n_valid or None, mask or None, grad_scale)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batches)))
        for widths, P, rows, target, nv, mk, scale in batches:
            B, R, _ = rows.shape
            f.write(struct.pack("<9if", *widths, B, R, int(nv is not None), int(mk is not None), float(scale)))
            f.write(np.ascontiguousarray(P, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(target, dtype="<f4").tobytes())
            if mk is not None:
                f.write(np.ascontiguousarray(mk, dtype="u1").tobytes())


def read_results(path, batches):
    raw, at, out = open(path, "rb").read(), 0, []
    for widths, P, rows, _, _, _, _ in batches:
        B, n = rows.shape[0], len(P)
        grad = np.frombuffer(raw, "<f4", n, at)
        at += 4 * n
        loss, count = struct.unpack_from("<dq", raw, at)
        at += 16
        value = np.frombuffer(raw, "<f4", B, at)
        at += 4 * B
        out.append((grad, loss, count, value, np.frombuffer(raw, "<i4", B, at)))
        at += 4 * B
    assert at == len(raw)
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plain_batch(widths, B, R, seed=None):
    """Ordinary states: (rows [B, R, T] float32, target [B] float32), rows like rotated joint states in size."""
    rs = np.random.RandomState(520000 + 1000 * widths[1] + 10 * B + R if seed is None else seed)
    return rs.normal(0.0, 1.0, (B, R, widths[0])).astype(np.float32), rs.normal(0.0, 0.5, (B,)).astype(np.float32)


def edge_batch(widths, B, R, seed=None):
    """plain_batch with a state of every kind of EDGE_KINDS in turn (state b has kind (b + R) % 9, so the shapes together
    cover them all at B = 1): (rows, target, n_valid [B] int64, mask [B] uint8, kinds [B]).
      tie            two rows with the same bytes hold the minimum (the later one's copy comes first: row 0 = row R - 1)
      ragged         1 <= n_valid < R        no_rows: n_valid 0        negative_rows: n_valid -3        rows_above: n_valid R + 5
      masked         mask 0, ordinary values        nan_masked: mask 0, NaN and infinities in its rows and its target
      nan_padding    n_valid < R and NaN, +inf, -inf in the rows past it
    Rows at or past n_valid of every state hold NaN, +inf and -inf in turn."""
    rows, target = plain_batch(widths, B, R, seed)
    rs = np.random.RandomState((7 if seed is None else seed) + 13 * B + R)
    nv, mask, kinds = np.full((B,), R, dtype=np.int64), np.ones((B,), dtype=np.uint8), []
    for b in range(B):
        kind = EDGE_KINDS[(b + R) % len(EDGE_KINDS)]
        kinds.append(kind)
        if kind == "tie":
            rows[b, 0] = rows[b, R - 1]
        elif kind in ("ragged", "nan_padding"):
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
            rows[b, rs.randint(R), rs.randint(widths[0])] = np.nan
            rows[b, rs.randint(R), 0] = np.inf
            target[b] = np.nan
        for r in range(max(0, min(R, int(nv[b]))), R):
            rows[b, r] = (np.nan, np.inf, -np.inf)[(r + b) % 3]
    return rows, target, nv, mask, kinds


def is_live(nv, mask):
    return (np.asarray(nv) >= 1) & (np.asarray(mask) != 0)


def torch_grad(sd, rows, target, n_valid, live, grad_scale, dtype):
    """torch autograd of CadrlModule in `dtype` on the float32 weights and the live states' float32 inputs (rows past
    n_valid zeroed: autograd multiplies them with zero deltas): (packed gradient as a float64 array, loss_sum, value [live])
    of grad_scale / 2 * the sum of squared differences."""
    from ebcsim.cadrl import CadrlModule
    from ebcsim.cadrl_train import pack_state_dict, widths_of
    m = CadrlModule.from_state_dict(sd).to(dtype)
    idx = np.nonzero(live)[0]
    x = np.array(np.asarray(rows)[idx], dtype=np.float32)
    R = x.shape[1]
    nv = None
    if n_valid is not None:
        nv = np.clip(np.asarray(n_valid)[idx], 0, R)
        x[np.arange(R)[None, :] >= nv[:, None]] = 0.0
        nv = torch.from_numpy(nv)
    v = m(torch.from_numpy(x).to(dtype), nv)
    d = v - torch.from_numpy(np.asarray(target, dtype=np.float32)[idx]).to(dtype)
    loss = (d * d).sum()
    (0.5 * float(grad_scale) * loss).backward()
    g = pack_state_dict({k: p.grad.to(torch.float64) for k, p in m.named_parameters()},
                        out=torch.zeros(host_floats(widths_of(sd)), dtype=torch.float64))
    return g.numpy(), float(loss.detach()), v.detach().double().numpy()


def row_values(sd, rows, dtype):
    """The network's output on every row [B, R] in `dtype`, as float64."""
    from ebcsim.cadrl import CadrlModule
    m = CadrlModule.from_state_dict(sd).to(dtype)
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(rows, dtype=np.float32)).to(dtype)
        return m.value_network(x.reshape(-1, x.shape[-1])).reshape(x.shape[0], x.shape[1]).double().numpy()


def accuracy_cases():
    return [(wi, B, R) for wi in range(len(WIDTHS)) for B in BATCHES for R in (1, 5)] + [(0, 100, 1), (0, 100, 5)]


_rows = {}
YARDSTICK_FLOOR = 2.0 ** -25
MAX_SEEDS = 2000


def reference_of(wi, B, R, seed):
    """What the comparison of one seeded batch needs and the code under test has no part in: the batch, float64 and
    float32 autograd of CadrlModule, torch's float32 error per layer and of the loss, the float64 top-2 gap of the rows'
    values and the tolerance of the values."""
    widths = WIDTHS[wi]
    sd = random_state_dict(widths)
    rows, target = plain_batch(widths, B, R, seed=530000 + 10007 * seed + 1000 * wi + 10 * B + R)
    v64, v32 = row_values(sd, rows, torch.float64), row_values(sd, rows, torch.float32)
    tol = TOL_FACTOR * float(np.abs(v32 - v64).max())
    gap = float(np.min(np.diff(np.sort(v64, axis=1)[:, :2], axis=1))) if R > 1 else float("inf")
    live, scale = np.ones(B, dtype=bool), 2.0 / B
    g64, l64, _ = torch_grad(sd, rows, target, None, live, scale, torch.float64)
    g32, l32, _ = torch_grad(sd, rows, target, None, live, scale, torch.float32)
    slices = layer_slices(widths)
    err32 = [float(np.abs(g32[s] - g64[s]).max() / np.abs(g64[s]).max()) for s in slices]
    return dict(widths=widths, sd=sd, rows=rows, target=target, scale=scale, g64=g64, l64=l64, err32=err32,
                loss32=abs(l32 - l64) / l64, gap=gap, tol=tol, pick64=np.argmin(v64, axis=1), slices=slices)


def usable(ref):
    """The two preconditions of a seed.  (1) Every state's float64 top-2 gap exceeds twice the tolerance of the values, so
    float32 and float64 take the minimum of the same row.  (2) The yardstick is one: torch's float32 error of every layer
    and of the loss is at least 2^-25 of the layer's largest entry, half the spacing of float32 numbers just below it,
    which is what rounding the exact result to float32 costs on average.  A draw in which torch's float32 result happens
    to land closer than that to the float64 one (it does for about one layer in ten: a layer of 5 weights has few entries
    to take a maximum over) measures luck, not float32 arithmetic, and 8 times it is no bar.  Neither condition looks at
    the rule's result."""
    return ref["gap"] > 2 * ref["tol"] and min(ref["err32"]) >= YARDSTICK_FLOOR and ref["loss32"] >= YARDSTICK_FLOOR


_refs = {}


def chosen_reference(wi, B, R):
    """reference_of the first seed (0, 1, ...) that is usable."""
    if (wi, B, R) not in _refs:
        for seed in range(MAX_SEEDS):
            ref = reference_of(wi, B, R, seed)
            if usable(ref):
                ref["seed"] = seed
                _refs[wi, B, R] = ref
                break
        else:
            raise AssertionError("no usable seed below %d for widths %s, B %d, R %d" % (MAX_SEEDS, WIDTHS[wi], B, R))
    return _refs[wi, B, R]


def accuracy_row(wi, B, R):
    """Per layer (name, err_rule, err_torch32), the loss's (err_rule, err_torch32), the precondition (smallest float64
    top-2 gap over the states, the tolerance of the values), the rows taken (rule, float64) and the seed, of the chosen
    seeded batch; computed once."""
    if (wi, B, R) not in _rows:
        from ebcsim.cadrl_train import LAYER_KEYS
        ref = chosen_reference(wi, B, R)
        g, loss, count, value, min_row = host_grad(host_pack(ref["sd"]), ref["widths"], ref["rows"], ref["target"], grad_scale=ref["scale"])
        assert count == B
        g64 = ref["g64"]
        layers = [(name, float(np.abs(g[s].astype(np.float64) - g64[s]).max() / np.abs(g64[s]).max()), e32)
                  for name, s, e32 in zip(LAYER_KEYS, ref["slices"], ref["err32"])]
        _rows[wi, B, R] = (layers, (abs(loss - ref["l64"]) / ref["l64"], ref["loss32"]), (ref["gap"], ref["tol"]),
                           (min_row, ref["pick64"]), ref["seed"])
    return _rows[wi, B, R]


def accuracy_table():
    lines = ["CADRL gradient rule (csrc/ebc_cadrl_grad_rule.h, host build) against torch autograd of CadrlModule in float64,",
             "beside torch's own float32 autograd: err = max |g - g_64| / max |g_64| per layer (W and bias together).",
             "EBC_CADRL_GRAD_CHUNK = %d.  Seeded networks and inputs of tests/cadrl_grad_cases.py; bar: rule <= %d x torch32."
             % (chunk(), TOL_FACTOR),
             "Per case the first seed whose float64 top-2 row gap exceeds twice the values' tolerance and whose torch32 errors are",
             "all at least 2^-25 (tests/cadrl_grad_cases.py: usable).", "",
             "%-22s %4s %3s  %-16s %11s %11s %7s" % ("widths", "B", "R", "layer", "err_rule", "err_torch32", "ratio")]
    ratio = lambda a, b: a / b if b else (float("inf") if a else 0.0)  # noqa: E731
    for wi, B, R in accuracy_cases():
        layers, (lr, lt), _, _, _ = accuracy_row(wi, B, R)
        name = "-".join(str(w) for w in WIDTHS[wi])
        for key, er, et in layers:
            lines.append("%-22s %4d %3d  %-16s %11.3e %11.3e %7.2f" % (name, B, R, key, er, et, ratio(er, et)))
        lines.append("%-22s %4d %3d  %-16s %11.3e %11.3e %7.2f" % (name, B, R, "loss_sum", lr, lt, ratio(lr, lt)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "cadrl_grad_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
