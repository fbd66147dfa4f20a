"""Shared by tests/test_sail_train_cpu.py and tests/test_sail_train_gpu.py: the host build of the SAIL gradient rule
(tests/native/sail_grad_host.cc: the source the kernel compiles, built with g++), seeded batches, torch's autograd of
SailModule as the reference, and the accuracy table both the test and profiles/sail_grad_accuracy.txt come from.

Bar.  The yardstick is the project's for the forward (profiles/sail_accuracy.txt): torch's own float32 autograd against
the same computation in float64 on the same float32 weights and inputs.  Per layer (its W and bias together)
err = max |g - g_64| / max |g_64|; the rule's error must stay within TOL_FACTOR times torch's float32 error.  Both are
float32 evaluations of the same sums: a serial fmaf chain of at most EBC_SAIL_GRAD_CHUNK * adult_num terms followed by
float64, against torch's blocked sums."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import torch

from sail_cases import random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "sail_grad_host.cc")
TOL_FACTOR = 8
ACCURACY_ADULTS = [2, 3, 5, 32]

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/sail_grad_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="sail_grad_host_")
        L = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libsail_grad_host.so")))
        L.sail_grad_host_chunk.restype = C.c_int
        L.sail_grad_host_group.restype, L.sail_grad_host_group.argtypes = C.c_int, [C.c_int]
        L.sail_grad_host_packed_floats.restype, L.sail_grad_host_packed_floats.argtypes = C.c_longlong, [C.c_int]
        L.sail_grad_host_pack.restype, L.sail_grad_host_pack.argtypes = None, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sail_grad_host.restype = None
        L.sail_grad_host.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 4
        _host["lib"] = L
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="sail_grad_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "sail_grad_host"))
    return _host[key]


def chunk():
    """EBC_SAIL_GRAD_CHUNK, from the header itself."""
    return int(host_lib().sail_grad_host_chunk())


def group(adult_num):
    """Envs the kernel's workgroup takes at once, from the header itself."""
    return int(host_lib().sail_grad_host_group(int(adult_num)))


def host_pack(sd):
    """The packed image of a state_dict by the header's own pack (float32 [packed_floats])."""
    from sail_cases import layer_arrays
    w, b = layer_arrays(sd)
    N = w[2].shape[1] // 4
    P = np.full(int(host_lib().sail_grad_host_packed_floats(N)), -7.0, dtype=np.float32)
    wp, bp = (C.c_void_p * 14)(*[a.ctypes.data for a in w]), (C.c_void_p * 14)(*[a.ctypes.data for a in b])
    host_lib().sail_grad_host_pack(N, wp, bp, P.ctypes.data)
    return P


def host_grad(P, N, robot, ob, target, n_rows=None, mask=None, grad_scale=1.0):
    """(grad float32 [packed_floats], loss_sum, count, action [E, 2]) of the host build on a packed image P."""
    robot, ob, target = (np.ascontiguousarray(a, dtype=np.float64) for a in (robot, ob, target))
    E, R = ob.shape[0], ob.shape[1]
    assert robot.shape == (E, 9) and ob.shape[2] == 5 and target.shape == (E, 2) and R >= N
    P = np.ascontiguousarray(P, dtype=np.float32)
    nr = None if n_rows is None else np.ascontiguousarray(n_rows, dtype=np.int64)
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    grad = np.full(P.shape, -7.0, dtype=np.float32)
    loss, count, action = C.c_double(-1.0), C.c_longlong(-1), np.full((E, 2), -7.0)
    host_lib().sail_grad_host(int(N), P.ctypes.data, robot.ctypes.data, ob.ctypes.data, None if nr is None else nr.ctypes.data,
                              target.ctypes.data, None if mk is None else mk.ctypes.data, float(grad_scale), E, R, grad.ctypes.data,
                              C.addressof(loss), C.addressof(count), action.ctypes.data)
    return grad, float(loss.value), int(count.value), action


def plain_batch(N, E, R, seed):
    """Ordinary states: (robot [E, 9], ob [E, R, 5], target [E, 2]); nobody has arrived (at least 0.5 from the goal, radius
    0.3); rows at or past N hold NaN, +inf and -inf in turn."""
    rs = np.random.RandomState(310000 + 1000 * N + 10 * E + R if seed is None else seed)
    robot = np.zeros((E, 9))
    robot[:, 0:2] = rs.uniform(-5, 5, (E, 2))
    robot[:, 2:4] = rs.uniform(-1, 1, (E, 2))
    robot[:, 4] = 0.3
    ang, dist = rs.uniform(0, 2 * np.pi, E), rs.uniform(0.5, 9.0, E)
    robot[:, 5], robot[:, 6] = robot[:, 0] + dist * np.cos(ang), robot[:, 1] + dist * np.sin(ang)
    robot[:, 7] = 1.0
    robot[:, 8] = rs.uniform(-3, 3, E)
    ob = np.zeros((E, R, 5))
    ob[:, :, 0:2] = rs.uniform(-5, 5, (E, R, 2))
    ob[:, :, 2:4] = rs.uniform(-1, 1, (E, R, 2))
    ob[:, :, 4] = 0.3
    for r in range(N, R):
        ob[:, r, :] = (np.nan, np.inf, -np.inf)[r % 3]
    return robot, ob, rs.uniform(-1, 1, (E, 2))


def masked_batch(N, E, R, seed, poison=True):
    """plain_batch with every kind of env that must not count, in turn: (robot, ob, target, n_rows, mask, live [E] bool).
    Env e is masked out (e % 4 == 1), ragged (e % 4 == 2, a row count other than N), arrived (e % 4 == 3, 0.14 from the
    goal) or live.  poison: the envs that do not count carry NaN and infinities in robot, in their rows and in target
    (an arrived env keeps its position and goal: they are what makes it arrived); else they hold ordinary values."""
    robot, ob, target = plain_batch(N, E, R, seed)
    rs = np.random.RandomState(seed + 1)
    n_rows, mask = np.full((E,), N, dtype=np.int64), np.ones((E,), dtype=np.uint8)
    for e in range(E):
        kind = e % 4
        if kind == 1:
            mask[e] = 0
        elif kind == 2:
            n_rows[e] = (N - 1, N + 1, 0, R + 4)[rs.randint(4)]
        elif kind == 3:
            robot[e, 5], robot[e, 6] = robot[e, 0] + 0.1, robot[e, 1] - 0.1
        row, col, out = rs.randint(N), rs.randint(4), rs.randint(2)  # drawn whether used or not: both forms share the rest
        if kind and poison:
            bad = (np.nan, np.inf, -np.inf)
            cols = (2, 3, 8) if kind == 3 else (0, 2, 5)
            for i, c in enumerate(cols):
                robot[e, c] = bad[(e + i) % 3]
            ob[e, row, col] = bad[e % 3]
            ob[e, 0, 0] = bad[(e + 1) % 3]
            target[e, out] = bad[(e + 2) % 3]
    return robot, ob, target, n_rows, mask, np.array([e % 4 == 0 for e in range(E)])


def torch_grad(sd, robot, ob, target, live, grad_scale, dtype):
    """torch autograd of SailModule in `dtype` on the float32 weights and the float32 casts of the live envs' inputs:
    (packed gradient as a float64 array, loss_sum) of grad_scale / 2 * sum of squared differences."""
    from ebcsim.sail import SailModule
    from ebcsim.sail_train import pack_state_dict
    m = SailModule.from_state_dict(sd).to(dtype)
    N = m.num_adult
    idx = np.nonzero(live)[0]
    # row-major like the trainer's (numpy's column selection alone comes out column-major, which torch's BLAS rounds differently)
    r = torch.from_numpy(np.ascontiguousarray(np.asarray(robot)[idx][:, [0, 1, 2, 3, 5, 6]].astype(np.float32))).to(dtype)
    c = torch.from_numpy(np.ascontiguousarray(np.asarray(ob)[idx][:, :N, :4]).astype(np.float32)).to(dtype)
    t = torch.from_numpy(np.asarray(target)[idx].astype(np.float32)).to(dtype)
    d = m(r, c)[0] - t
    loss = (d * d).sum()
    (0.5 * float(grad_scale) * loss).backward()
    g = pack_state_dict({k: p.grad.to(torch.float64) for k, p in m.named_parameters()},
                        out=torch.zeros(int(host_lib().sail_grad_host_packed_floats(N)), dtype=torch.float64))
    return g.numpy(), float(loss.detach())


def layer_slices(N):
    from ebcsim.sail_train import layer_shapes
    out, at = [], 0
    for k, _ in layer_shapes(N):
        out.append(slice(at, at + (k + 1) * 64))
        at += (k + 1) * 64
    return out


def accuracy_cases():
    Cn = chunk()
    return [(N, E) for N in ACCURACY_ADULTS for E in (1, Cn - 1, Cn, Cn + 1, 2 * Cn + 3)] + [(5, 256)]


_rows = {}


def accuracy_row(N, E):
    """Per layer (err_rule, err_torch32), and the loss's (err_rule, err_torch32), of one seeded batch; computed once."""
    if (N, E) not in _rows:
        from ebcsim.sail import LAYERS
        sd = random_state_dict(N, 8)
        robot, ob, target = plain_batch(N, E, N, None)
        live = np.ones(E, dtype=bool)
        scale = 1.0 / E
        g, loss, count, _ = host_grad(host_pack(sd), N, robot, ob, target, grad_scale=scale)
        assert count == E
        g64, l64 = torch_grad(sd, robot, ob, target, live, scale, torch.float64)
        g32, l32 = torch_grad(sd, robot, ob, target, live, scale, torch.float32)
        layers = []
        for name, s in zip(LAYERS, layer_slices(N)):
            top = np.abs(g64[s]).max()
            layers.append((name, float(np.abs(g[s].astype(np.float64) - g64[s]).max() / top), float(np.abs(g32[s] - g64[s]).max() / top)))
        _rows[N, E] = (layers, (abs(loss - l64) / l64, abs(l32 - l64) / l64))
    return _rows[N, E]


def accuracy_table():
    lines = ["SAIL gradient rule (csrc/ebc_sail_grad_rule.h, host build) against torch autograd of SailModule in float64,",
             "beside torch's own float32 autograd: err = max |g - g_64| / max |g_64| per layer (W and bias together).",
             "EBC_SAIL_GRAD_CHUNK = %d.  Seeded weights (attention x8) and inputs of tests/sail_grad_cases.py; bar: rule <= %d x torch32."
             % (chunk(), TOL_FACTOR), "",
             "%3s %4s  %-18s %11s %11s %7s" % ("N", "E", "layer", "err_rule", "err_torch32", "ratio")]
    for N, E in accuracy_cases():
        layers, (lr, lt) = accuracy_row(N, E)
        for name, er, et in layers:
            lines.append("%3d %4d  %-18s %11.3e %11.3e %7.2f" % (N, E, name, er, et, er / et if et else float("inf") if er else 0.0))
        lines.append("%3d %4d  %-18s %11.3e %11.3e %7.2f" % (N, E, "loss_sum", lr, lt, lr / lt if lt else float("inf") if lr else 0.0))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "sail_grad_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
