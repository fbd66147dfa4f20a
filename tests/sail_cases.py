"""Shared by tests/test_sail_cpu.py and tests/test_sail_gpu.py: the golden SAIL run and constructed states, the host build
of the network (tests/native/sail_host.cc: the source the kernel compiles, built with g++), the edge batches, and the one
tolerance both files hold.

Tolerance.  The yardstick is torch's own float32 arithmetic against the same computation in float64 on the same float32
weights and inputs: e_ref = max |ExtendedNetwork float32 - its float64 copy| over every recorded input of a golden file,
measured by the tests, separately for `action` and for `feat_joint`.  Recorded actions and features are held to
TOL_FACTOR * e_ref, the rule already used for LSTM-RL and CADRL: a serial fmaf chain of at most 128 terms and torch's
blocked sums are both float32 evaluations of the same sum."""
import ctypes as C
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "sail_host.cc")
TOL_FACTOR = 8
ADULTS = [2, 5, 32]
TILE_ROWS = 5  # EBC_SAIL_T of csrc/ebc_sail.h: the rows a wave carries at once
KINDS = ["plain", "ragged", "arrived", "nan_valid", "equal_logits", "arrived_ragged", "still"]

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/sail_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="sail_host_")
        _host["lib"] = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libsail_host.so")))
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="sail_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "sail_host"))
    return _host[key]


def host_group(adult_num):
    """Envs per workgroup of the kernel, from the header itself."""
    fn = host_lib().sail_host_group
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    return int(fn(int(adult_num)))


def layer_arrays(sd):
    """(weights, biases) of a state_dict as contiguous float32 arrays in the order of EbcSailWeights."""
    from ebcsim.sail import LAYERS
    get = lambda k: np.ascontiguousarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float32)  # noqa: E731
    return [get(k + ".weight") for k in LAYERS], [get(k + ".bias") for k in LAYERS]


def host_forward(sd, robot, ob, n_rows=None, want_feat=True):
    """(action [E, 2] float64, feat_joint [E, 64] float32) of the host build: robot [E, 9], ob [E, R, 5] float64."""
    robot, ob = np.ascontiguousarray(robot, dtype=np.float64), np.ascontiguousarray(ob, dtype=np.float64)
    E, R = ob.shape[0], ob.shape[1]
    assert robot.shape == (E, 9) and ob.shape[2] == 5
    w, b = layer_arrays(sd)
    N = w[2].shape[1] // 4
    assert R >= N
    nr = None if n_rows is None else np.ascontiguousarray(n_rows, dtype=np.int64)
    action, feat = np.full((E, 2), -7.0), np.full((E, 64), -7.0, dtype=np.float32)
    wp, bp = (C.c_void_p * 14)(*[a.ctypes.data for a in w]), (C.c_void_p * 14)(*[a.ctypes.data for a in b])
    fn = host_lib().sail_host
    fn.restype = None
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fn(N, wp, bp, robot.ctypes.data, ob.ctypes.data, None if nr is None else nr.ctypes.data, E, R, action.ctypes.data,
       feat.ctypes.data if want_feat else None)
    return action, feat


def write_batches(path, batches):
    """The input file of the host program (the format is in sail_host.cc): batches of (sd, robot, ob, n_rows or None)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batches)))
        for sd, robot, ob, nr in batches:
            w, b = layer_arrays(sd)
            E, R = ob.shape[0], ob.shape[1]
            f.write(struct.pack("<iiii", w[2].shape[1] // 4, E, R, int(nr is not None)))
            for wl, bl in zip(w, b):
                f.write(wl.astype("<f4").tobytes())
                f.write(bl.astype("<f4").tobytes())
            f.write(np.ascontiguousarray(robot, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(ob, dtype="<f8").tobytes())
            if nr is not None:
                f.write(np.ascontiguousarray(nr, dtype="<i8").tobytes())


def read_results(path, batches):
    raw, at, out = open(path, "rb").read(), 0, []
    for _, _, ob, _ in batches:
        E = ob.shape[0]
        action = np.frombuffer(raw, "<f8", E * 2, at).reshape(E, 2)
        at += 16 * E
        out.append((action, np.frombuffer(raw, "<f4", E * 64, at).reshape(E, 64)))
        at += 256 * E
    assert at == len(raw)
    return out


_weights = {}


def random_state_dict(adult_num, scale=1):
    """Seeded random weights of SailModule(adult_num) (torch's own initialisation); scale multiplies the weights of the two
    attention layers, so that the logits spread by scale^2 and the softmax is not flat."""
    key = (adult_num, scale)
    if key not in _weights:
        from ebcsim.sail import SailModule
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(1000 + adult_num)
            sd = {k: v.detach().clone() for k, v in SailModule(adult_num).state_dict().items()}
        for k in ("attention.0.weight", "attention.2.weight"):
            sd[k] = sd[k] * float(scale)
        _weights[key] = sd
    return _weights[key]


def env_counts(adult_num):
    """The env counts a shape is tested at: 1, G - 1, G, G + 1, 2 G + 1 for the kernel's G envs per workgroup, and one
    whose last workgroup ends in a tile of fewer than TILE_ROWS rows where the shape allows one; and 7, an env of every
    kind of KINDS."""
    G = host_group(adult_num)
    out = [1, G - 1, G, G + 1, 2 * G + 1, len(KINDS)]
    for E in range(G + 1, 3 * G + 1):
        last = (E % G or G) * adult_num
        if last % TILE_ROWS:
            out.append(E)
            break
    return sorted({E for E in out if E >= 1})


def edge_batch(adult_num, E, R, seed=None):
    """One batch with every edge in turn, an env per kind of KINDS (a one-env batch takes the kind (adult_num + R) % 7)
    -> (robot [E, 9], ob [E, R, 5], n_rows [E] int64, kinds [E]).  Padding rows (at or past adult_num) hold NaN, +inf and
    -inf in turn; ragged envs have a row count other than adult_num; arrived envs stand 0.14 from the goal with radius
    0.3, every other env at least 0.5; nan_valid has a NaN inside a valid row; equal_logits has adult_num identical
    agents (identical rows of the network, so identical logits); still has zero velocities everywhere."""
    N = adult_num
    rs = np.random.RandomState(200000 + 1000 * N + 10 * E + R if seed is None else seed)
    robot = np.zeros((E, 9))
    robot[:, 0:2] = rs.uniform(-5, 5, (E, 2))
    robot[:, 2:4] = rs.uniform(-1, 1, (E, 2))
    robot[:, 4] = 0.3
    ang = rs.uniform(0, 2 * np.pi, E)
    dist = rs.uniform(0.5, 9.0, E)
    robot[:, 5], robot[:, 6] = robot[:, 0] + dist * np.cos(ang), robot[:, 1] + dist * np.sin(ang)
    robot[:, 7] = 1.0
    robot[:, 8] = rs.uniform(-3, 3, E)
    ob = np.zeros((E, R, 5))
    ob[:, :, 0:2] = rs.uniform(-5, 5, (E, R, 2))
    ob[:, :, 2:4] = rs.uniform(-1, 1, (E, R, 2))
    ob[:, :, 4] = 0.3
    for r in range(N, R):
        ob[:, r, :] = (np.nan, np.inf, -np.inf)[r % 3]
    n_rows = np.full((E,), N, dtype=np.int64)
    kinds = []
    for e in range(E):
        kind = KINDS[((N + R) if E == 1 else (e + N)) % len(KINDS)]
        kinds.append(kind)
        if kind in ("ragged", "arrived_ragged"):
            n_rows[e] = (N - 1, N + 1, 0, R + 4)[rs.randint(4)]
        if kind in ("arrived", "arrived_ragged"):
            robot[e, 5], robot[e, 6] = robot[e, 0] + 0.1, robot[e, 1] - 0.1
        if kind == "nan_valid":
            ob[e, rs.randint(N), rs.randint(4)] = np.nan
        if kind == "equal_logits":
            ob[e, :N] = ob[e, 0]
        if kind == "still":
            robot[e, 2:4] = 0.0
            ob[e, :N, 2:4] = 0.0
    return robot, ob, n_rows, kinds


def check_kinds(action, feat, n_rows, kinds, adult_num, tag=""):
    """What every kind promises, whoever computed it."""
    for e, kind in enumerate(kinds):
        where = (tag, e, kind)
        if kind in ("ragged", "arrived_ragged"):
            assert n_rows[e] != adult_num and np.isnan(action[e]).all() and (feat[e] == 0).all(), where
        elif kind == "arrived":
            assert (action[e] == 0).all() and np.isfinite(feat[e]).all() and feat[e].any(), where
        elif kind == "nan_valid":
            assert np.isnan(action[e]).all(), where
        else:
            assert np.isfinite(action[e]).all() and np.isfinite(feat[e]).all() and action[e].any(), where


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_golden = {}


def golden(name):
    """(z, meta, state_dict, SailModule float32, its float64 copy) of a golden file, built once; the recorded state_dict
    (arrays under "sd/<key>", in the reference's own key order) loads with strict=True."""
    if name not in _golden:
        from ebcsim.sail import SailModule
        z = load(name)
        meta = json.loads(str(z["meta"]))
        sd = {k: torch.from_numpy(z["sd/" + k].copy()) for k in meta["state_dict"]}
        _golden[name] = (z, meta, sd, SailModule.from_state_dict(sd).eval(), SailModule.from_state_dict(sd).double().eval())
    return _golden[name]


def network_inputs(robot, ob, adult_num):
    """The casts of SAIL.transform on float64 states: (robot_state [E, 6], crowd [E, N, 4]) float32 tensors."""
    robot, ob = np.asarray(robot, dtype=np.float64), np.asarray(ob, dtype=np.float64)
    return (torch.from_numpy(robot[:, [0, 1, 2, 3, 5, 6]].astype(np.float32)),
            torch.from_numpy(np.ascontiguousarray(ob[:, :adult_num, :4]).astype(np.float32)))


def ref_error(m32, m64, robot, ob):
    """e_ref of a set of states: (max |action32 - action64|, max |feat_joint32 - feat_joint64|)."""
    r, c = network_inputs(robot, ob, m32.num_adult)
    with torch.no_grad():
        a32, f32 = m32(r, c)
        a64, f64 = m64(r.double(), c.double())
    return float((a32.double() - a64).abs().max()), float((f32.double() - f64).abs().max())


def golden_weights_file(sd, directory):
    """The state_dict as a file torch.save wrote (what a training run leaves), in `directory` (a test's tmp_path)."""
    path = os.path.join(str(directory), "sail_model.pth")
    torch.save({k: v.clone() for k, v in sd.items()}, path)
    return path
