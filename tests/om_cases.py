"""Shared by tests/test_om_cpu.py and tests/test_om_gpu.py: the goldens of the occupancy maps (tests/golden/om_cases.npz,
the reference's own build_occupancy_maps on constructed states) and of OM-SARL (tests/golden/om_sarl_*.npz, the reference's
own SARL with with_om = true), the host build of the rule (tests/native/om_host.cc: the source the kernel compiles, built
with g++), the edge batches, and the tolerances both files hold.

Tolerances.  The product states the reference's arctan2 / cos / sin frame algebraically (csrc/ebc_om_rule.h).  The two forms
differ by float64 rounding only, so (i) a cell is the same cell unless a coordinate lies on a boundary to within that
rounding — the goldens' generator refuses any state with a non-coincident pair within MARGIN cells of one, and the tests
assert that none is left out; (ii) a mean velocity, cast to float32 once, can at most be the neighbouring float32:
one spacing of the recorded value, plus VEL_ABS for a cancelled component the reference leaves at 1e-17 instead of 0.
The network's values are held to TOL_FACTOR x the error of torch's own float32 forward against a float64 copy of the same
module on the same rows (the bar of tests/test_cadrl_cpu.py), measured by the tests."""
import ctypes as C
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import torch

from ebcsim import _abi
from ebcsim.occupancy import OccupancySpec
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "om_host.cc")
RUNS = ["om_sarl_a5_c3", "om_sarl_n10_c3", "om_sarl_n10_c1"]
TOL_FACTOR = 8
MARGIN = 1e-9
VEL_ABS = 1e-12
ENVS = [1, 3, 65]
ROWS = [1, 2, 18, 33, 128]
ACTIONS = [1, 2, 81]
WIDTHS = [13, 17]
GRIDS = [(4, 3), (4, 1), (3, 2), (8, 3)]  # (cell_num, channels)
CELL_SIZE = {4: 1.0, 3: 0.5, 8: 1.0}
MAX_WIDE_FLOATS = 48 << 20  # the largest rows_wide a shape of the sweep may have (192 MB): larger ones take fewer actions

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/om_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="om_host_")
        lib = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libom_host.so")))
        lib.om_host.restype = None
        lib.om_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                C.c_int, C.c_void_p, C.c_void_p]
        _host["lib"] = lib
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="om_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "om_host"))
    return _host[key]


def host_om(next_ob, n_valid, spec, rows=None):
    """(om [E, R, W] float32, rows_wide [E, A, R, T + W] or None) of the host build."""
    ob = np.ascontiguousarray(next_ob, dtype=np.float64)
    E, R = ob.shape[:2]
    assert ob.shape[2] == 5
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    om = np.full((E, R, spec.width), np.float32(-7.0))
    A = T = 0
    wide = None
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        A, T = rows.shape[1], rows.shape[3]
        assert rows.shape == (E, A, R, T)
        wide = np.full((E, A, R, T + spec.width), np.float32(-7.0))
    host_lib().om_host(ob.ctypes.data, None if nv is None else nv.ctypes.data, None if rows is None else rows.ctypes.data,
                       E, A, R, T, spec.cell_num, spec.cell_size, spec.channels, om.ctypes.data,
                       None if wide is None else wide.ctypes.data)
    return om, wide


def write_batches(path, batches):
    """The input file of the host program (the format is in om_host.cc): batches of (next_ob, n_valid or None, spec, rows or None)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batches)))
        for ob, nv, spec, rows in batches:
            E, R = ob.shape[:2]
            A, T = (rows.shape[1], rows.shape[3]) if rows is not None else (0, 0)
            f.write(struct.pack("<iiiiiiiid", E, A, R, T, spec.cell_num, spec.channels, int(nv is not None), int(rows is not None),
                                spec.cell_size))
            f.write(np.ascontiguousarray(ob, dtype="<f8").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            if rows is not None:
                f.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())


def read_results(path, batches):
    raw, at, out = open(path, "rb").read(), 0, []
    for ob, _, spec, rows in batches:
        E, R = ob.shape[:2]
        om = np.frombuffer(raw, "<f4", E * R * spec.width, at).reshape(E, R, spec.width)
        at += om.nbytes
        wide = None
        if rows is not None:
            shape = rows.shape[:3] + (rows.shape[3] + spec.width,)
            wide = np.frombuffer(raw, "<f4", int(np.prod(shape)), at).reshape(shape)
            at += wide.nbytes
        out.append((om, wide))
    assert at == len(raw)
    return out


def golden_cases():
    """[(ob [R, 5] float64, spec, kind name, the reference's maps [R, W] float32)] of tests/golden/om_cases.npz."""
    if "cases" not in _host:
        z = load("om_cases")
        kinds = json.loads(str(z["meta"]))["kinds"]
        out = []
        for i in range(len(z["rows"])):
            R = int(z["rows"][i])
            spec = OccupancySpec(z["cell_num"][i], z["cell_size"][i], z["channels"][i])
            want = z["maps"][z["offsets"][i]:z["offsets"][i + 1]].reshape(R, spec.width)
            out.append((np.ascontiguousarray(z["ob"][i, :R]), spec, kinds[int(z["kind"][i])], want))
        _host["cases"] = out
    return _host["cases"]


def velocity_columns(spec):
    """Boolean [W]: the columns of a map that hold a mean velocity (the others hold the occupancy 0 / 1)."""
    col = np.arange(spec.width) % spec.channels
    return np.zeros(spec.width, bool) if spec.channels == 1 else (col >= spec.channels - 2)


def compare_maps(got, want, spec):
    """Occupancy columns equal; velocity columns within one float32 spacing of the recorded value plus VEL_ABS -> the largest
    velocity difference in units of that bound's spacing part (0 for equal maps)."""
    vel = velocity_columns(spec)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got[..., ~vel], want[..., ~vel])
    d = np.abs(got[..., vel].astype(np.float64) - want[..., vel].astype(np.float64))
    bound = np.spacing(np.abs(want[..., vel])).astype(np.float64) + VEL_ABS
    assert (d <= bound).all(), (float(d.max()), float((d / bound).max()))
    return float(d.max()) if d.size else 0.0


def shape_sweep(grid_index):
    """The (E, R, A, T) shapes of one (cell_num, channels): every E x R, the action counts and row widths in turn so that
    every A and every T meets every E, every R and every grid; a shape whose rows_wide would exceed MAX_WIDE_FLOATS takes
    the next smaller action count."""
    cell_num, channels = GRIDS[grid_index]
    W = cell_num * cell_num * channels
    out = []
    for i, E in enumerate(ENVS):
        for j, R in enumerate(ROWS):
            T = WIDTHS[(i + j + grid_index) % 2]
            k = (i + j + grid_index) % 3
            while E * ACTIONS[k] * R * (T + W) > MAX_WIDE_FLOATS:
                k -= 1
            out.append((E, R, ACTIONS[k], T))
    return out


def edge_batch(E, R, A, T, cell_num, channels, seed=None):
    """(next_ob [E, R, 5] float64, n_valid [E] int64, rows [E, A, R, T] float32, spec): ragged n_valid holding 0, 1 and R
    (and values above R and below 0), NaN in every row at or past n_valid, occupants inside and far outside the grid,
    coincident rows, standing rows with zero velocities of both signs, and rows whose float32 payload includes NaN
    and infinity bit patterns (they are copied, never computed with)."""
    spec = OccupancySpec(cell_num, CELL_SIZE[cell_num], channels)
    rs = np.random.RandomState(7000000 + 100000 * cell_num + 10000 * channels + 1000 * E + 10 * R + A + T if seed is None else seed)
    half = 0.5 * cell_num * spec.cell_size
    ob = np.zeros((E, R, 5))
    ob[:, :, :2] = rs.uniform(-1.4 * half, 1.4 * half, (E, R, 2))
    ob[:, :, 2:4] = rs.normal(0.0, 0.8, (E, R, 2))
    ob[:, :, 4] = 0.3
    far = rs.uniform(size=(E, R)) < 0.1
    ob[far, :2] *= 1e3
    still = rs.uniform(size=(E, R)) < 0.25
    zeros = np.array([[0.0, 0.0], [0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0]])
    ob[still, 2:4] = zeros[rs.randint(4, size=int(still.sum()))]
    if R > 1:
        for e in range(E):
            for _ in range(1 + R // 8):
                i, j = rs.permutation(R)[:2]
                ob[e, j, :2] = ob[e, i, :2]
    nv = rs.randint(0, R + 1, size=E).astype(np.int64)
    special = [0, 1, R, R + 3, -2]
    for e in range(min(E, len(special))):
        nv[(e * 7) % E if E > len(special) else e] = special[e]
    if E == 1:
        nv[0] = (R, 1, 0)[(R + A + cell_num) % 3]
    for e in range(E):
        ob[e, max(0, min(R, int(nv[e]))):] = np.nan
    rows = rs.normal(0.0, 2.0, (E, A, R, T)).astype(np.float32)
    flat = rows.reshape(-1).view(np.uint32)
    flat[rs.randint(flat.size, size=max(1, flat.size // 97))] = np.array([0x7fc01234, 0xff800000, 0x7f800000, 0x80000000],
                                                                          dtype=np.uint32)[rs.randint(4, size=max(1, flat.size // 97))]
    return ob, nv, rows, spec


def tensor_digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def golden_state_dict(meta):
    """The network of a golden run, as its generator made it: the module the run's policy config describes (mlp1 T + W
    wide), built after torch.manual_seed(meta["torch_seed"]) (no tree ships OM weights and the goldens carry none) -> a
    state_dict with the reference's keys, every tensor held to the name, shape and SHA-256 recorded from the reference's own
    get_model().state_dict()."""
    import configparser
    from ebcsim.train import SarlModule
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["policy_config_text"])
    dims = lambda key: [int(x) for x in cfg.get("sarl", key).split(", ")]  # noqa: E731
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(meta["torch_seed"]))
        m = SarlModule(int(meta["input_dim"]), dims("mlp1_dims"), dims("mlp2_dims"), dims("mlp3_dims"), dims("attention_dims"),
                       cfg.getboolean("sarl", "with_global_state"), 6)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    want = meta["state_dict"]
    assert list(sd) == [k for k, _, _ in want], (list(sd), [k for k, _, _ in want])
    for k, shape, digest in want:
        assert list(sd[k].shape) == shape and sd[k].dtype == torch.float32, k
        assert tensor_digest(sd[k]) == digest, "%s: this torch does not rebuild the recorded tensor from seed %d" % (k, meta["torch_seed"])
    return sd


def golden_weights_file(meta, directory):
    """The same state_dict as a file torch.save wrote (what rl/train.py leaves), in `directory` (a test's tmp_path)."""
    path = os.path.join(str(directory), "rl_model.bin")
    torch.save(golden_state_dict(meta), path)
    return path


_runs = {}


def golden_run(name):
    """(z, meta, spec, SarlValueNet float32 on the CPU, its float64 copy) of a golden run, built once."""
    if name not in _runs:
        from ebcsim.sarl import SarlValueNet
        z = load(name)
        meta = json.loads(str(z["meta"]))
        sd = golden_state_dict(meta)
        spec = OccupancySpec(meta["cell_num"], meta["cell_size"], meta["channels"])
        n32 = SarlValueNet(sd, with_global_state=meta["with_global_state"])
        n64 = SarlValueNet(sd, with_global_state=meta["with_global_state"], dtype=torch.float64)
        _runs[name] = (z, meta, spec, n32, n64)
    return _runs[name]


def value_error(n32, n64, rows):
    """max |network float32 - its float64 copy| over the joint states rows [B, R, T + W] (a float32 tensor)."""
    x = rows.reshape(-1, rows.shape[-2], rows.shape[-1]).cpu()
    return float((n32.forward(x, exact=True).double() - n64.forward(x.double(), exact=True).double()).abs().max())


def chosen_index(z, t):
    return int(np.where((z["action_space"] == z["action"][t]).all(1))[0][0])


def om_args(E=1, A=1, R=2, T=13, cell_num=4, channels=3, cell_size=1.0, size=None, **ptrs):
    buf = om_args.buf.ctypes.data
    a = _abi.EbcOmArgs()
    a.struct_size = C.sizeof(a) if size is None else size
    a.E, a.A, a.R, a.T, a.cell_num, a.channels, a.cell_size = E, A, R, T, cell_num, channels, cell_size
    for k in ("next_ob", "rows", "om", "rows_wide"):
        setattr(a, k, ptrs.get(k, buf))
    a.n_valid = ptrs.get("n_valid", None)
    return a


om_args.buf = np.zeros(8, dtype=np.float64)

REFUSALS = [(dict(channels=0), b"channels"), (dict(channels=4), b"channels"), (dict(cell_num=0), b"cell_num < 1"),
            (dict(cell_num=9, channels=3), b"W > 192"), (dict(cell_num=8, channels=3, T=33), b"T + W > 224"),
            (dict(R=129), b"R > 128"), (dict(A=129), b"A > 128"), (dict(cell_size=0.0), b"cell_size"),
            (dict(cell_size=-1.0), b"cell_size"), (dict(cell_size=float("inf")), b"cell_size"),
            (dict(cell_size=float("nan")), b"cell_size"), (dict(om=None, rows_wide=None), b"no output"),
            (dict(rows=None), b"rows_wide without rows")]
