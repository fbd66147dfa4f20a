"""Shared by tests/test_cadrl_cpu.py and tests/test_cadrl_gpu.py: the golden CADRL runs, the host build of the decision
rule (tests/native/cadrl_host.cc: the source the decision kernel compiles, built with g++), a plain torch restatement of
the same rule, the edge batches, and the one tolerance both files hold.

Tolerance.  The yardstick is torch's own float32 arithmetic against the same computation in float64 on the same float32
weights and inputs: e_ref = max |value_network float32 - its float64 copy| over every row of a run's look-ahead rows,
measured by the tests.  A run's values are held to TOL_FACTOR * e_ref, the rule already used for LSTM-RL.  The goldens'
generator asserts that every run's smallest top-2 gap exceeds twice that, so no decision is left out of a comparison."""
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
SOURCE = os.path.join(ROOT, "tests", "native", "cadrl_host.cc")
RUNS = ["cadrl_a5", "cadrl_n10", "cadrl_one"]
TOL_FACTOR = 8
ENVS = [1, 3, 65]
ACTIONS = [1, 2, 63, 64, 65, 81, 128]
ROWS = [1, 2, 18, 33]
KINDS = ["full", "ragged", "nan_valid", "all_nan", "no_rows", "tie_halves", "inf_valid", "tie_inside"]

_host = {}


def _build(extra, out):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [SOURCE, "-o", out],
                   check=True, timeout=300)
    return out


def host_lib():
    """tests/native/cadrl_host.cc as a shared library, built once per process."""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="cadrl_host_")
        _host["lib"] = C.CDLL(_build(["-fPIC", "-shared"], os.path.join(d, "libcadrl_host.so")))
    return _host["lib"]


def host_program(sanitize=False):
    """The same file as a program of its own; sanitize: -fsanitize=address,undefined, no recovery from a finding."""
    key = "program_san" if sanitize else "program"
    if key not in _host:
        d = tempfile.mkdtemp(prefix="cadrl_host_")
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
        _host[key] = _build(flags, os.path.join(d, "cadrl_host"))
    return _host[key]


def host_decide(v, n_valid, reward, discount):
    """(values [E, A] float64, choice [E] int32) of the host build: v [E, A, R] float32, n_valid [E] int64 or None."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    E, A, R = v.shape
    reward = np.ascontiguousarray(reward, dtype=np.float64)
    assert reward.shape == (E, A)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int64)
    values, choice = np.full((E, A), -7.0), np.full((E,), -7, dtype=np.int32)
    fn = host_lib().cadrl_host
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fn(v.ctypes.data, None if nv is None else nv.ctypes.data, reward.ctypes.data, float(discount), E, A, R,
       values.ctypes.data, choice.ctypes.data)
    return values, choice


def write_batches(path, batches):
    """The input file of the host program (the format is in cadrl_host.cc)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(batches)))
        for v, nv, reward, discount in batches:
            E, A, R = v.shape
            f.write(struct.pack("<iiiid", E, A, R, int(nv is not None), float(discount)))
            f.write(np.ascontiguousarray(v, dtype="<f4").tobytes())
            if nv is not None:
                f.write(np.ascontiguousarray(nv, dtype="<i8").tobytes())
            f.write(np.ascontiguousarray(reward, dtype="<f8").tobytes())


def read_results(path, batches):
    raw, at, out = open(path, "rb").read(), 0, []
    for v, _, _, _ in batches:
        E, A, _ = v.shape
        values = np.frombuffer(raw, "<f8", E * A, at).reshape(E, A)
        at += 8 * E * A
        out.append((values, np.frombuffer(raw, "<i4", E, at)))
        at += 4 * E
    assert at == len(raw)
    return out


def restated(v, n_valid, reward, discount):
    """The rule in plain torch and Python, as the reference runs it (cadrl.py:192-217): torch.min over the rows that
    exist, reward + discount * min in Python floats, `if min_value > max_min_value` from -inf; -1 for max_action None,
    and NaN for a state without rows (where the reference's torch.cat raises)."""
    E, A, R = v.shape
    values, choice = np.zeros((E, A)), np.zeros((E,), np.int32)
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    for e in range(E):
        n = R if n_valid is None else max(0, min(R, int(n_valid[e])))
        best, pick = float("-inf"), -1
        for a in range(A):
            m = float(torch.min(t[e, a, :n], 0)[0]) if n else float("nan")
            value = float(reward[e, a]) + float(discount) * m
            values[e, a] = value
            if value > best:
                best, pick = value, a
        choice[e] = pick
    return values, choice


def edge_batch(E, A, R, seed=None):
    """One batch of a shape with every edge the shape has room for, an env per kind of KINDS in turn (a one-env batch
    takes the kind (A + R) % 8, so the shapes together cover them all) -> (v [E, A, R] float32, n_valid [E] int64,
    reward [E, A] float64, discount, kinds [E]).  Padding rows hold NaN, -inf and +inf in turn; n_valid holds 0, 1, R,
    values above R and below 0; ties are exact (equal rows and equal rewards) and are the env's best value."""
    rs = np.random.RandomState(100000 + 1000 * E + 10 * A + R if seed is None else seed)
    v = rs.normal(0.0, 1.5, (E, A, R)).astype(np.float32)
    reward = np.round(rs.normal(0.0, 0.3, (E, A)), 2)
    nv = np.full((E,), R, dtype=np.int64)
    kinds = []
    for e in range(E):
        kind = KINDS[((A + R) if E == 1 else (e + A)) % len(KINDS)]
        kinds.append(kind)
        if kind == "full":
            nv[e] = R + 5
        elif kind == "ragged":
            nv[e] = rs.randint(1, R + 1)
        elif kind == "nan_valid":
            nv[e] = rs.randint(1, R + 1)
            hit = rs.uniform(size=A) < 0.4
            hit[rs.randint(A)] = True
            if A > 1:
                hit[rs.randint(A)] = False
            v[e, hit, rs.randint(nv[e])] = np.nan
        elif kind == "all_nan":
            nv[e] = rs.randint(1, R + 1)
            v[e, np.arange(A), rs.randint(nv[e], size=A)] = np.nan
        elif kind == "no_rows":
            nv[e] = 0 if e % 2 == 0 else -3
        elif kind in ("tie_halves", "tie_inside"):
            nv[e] = 1 if kind == "tie_inside" else rs.randint(1, R + 1)
            if A > 1:
                if kind == "tie_halves" and A > 64:
                    lo = rs.randint(A - 64)
                    pair = (lo, lo + 64)
                else:
                    lo = rs.randint(min(A, 64) - 1)
                    pair = (lo, rs.randint(lo + 1, min(A, 64)))
                v[e, pair[1]] = v[e, pair[0]] = np.float32(50.0) + v[e, pair[0]]
                reward[e, pair[1]] = reward[e, pair[0]]
        elif kind == "inf_valid":
            nv[e] = R
            v[e, rs.randint(A), rs.randint(R)] = -np.inf
            v[e, rs.randint(A), :] = np.inf
            if A > 2:
                reward[e, rs.randint(A)] = -np.inf
        n = max(0, min(R, int(nv[e])))
        for r in range(n, R):
            v[e, :, r] = (np.nan, -np.inf, np.inf)[(r + e) % 3]
    return v, nv, reward, 0.9 ** (0.25 * (1.0 + 0.1 * (A % 3))), kinds


def all_edge_batches():
    """(E, A, R) -> edge_batch(E, A, R) for every shape of ENVS x ACTIONS x ROWS."""
    if "edges" not in _host:
        _host["edges"] = {(E, A, R): edge_batch(E, A, R) for E in ENVS for A in ACTIONS for R in ROWS}
    return _host["edges"]


def same_values(a, b):
    """Equal float64 arrays, NaN equal to NaN, +0 equal to -0."""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def tensor_digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def golden_state_dict(meta):
    """The network of a golden run, as its generator made it: the module the run's policy config describes, built after
    torch.manual_seed(meta["torch_seed"]) (neither tree ships a trained CADRL model and the goldens carry none: the
    recorded values hold this construction to the reference's) -> a state_dict with the reference's keys, every tensor
    held to the name, shape and SHA-256 recorded from the reference's own get_model().state_dict()."""
    import configparser
    from ebcsim.cadrl import CadrlModule
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["policy_config_text"])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(meta["torch_seed"]))
        m = CadrlModule(13, [int(x) for x in cfg.get("cadrl", "mlp_dims").split(", ")])
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
    """(z, meta, CadrlModule float32, its float64 copy) of a golden run, built once; the state_dict loads with strict=True."""
    if name not in _runs:
        from ebcsim.cadrl import CadrlModule
        z = load(name)
        meta = json.loads(str(z["meta"]))
        sd = golden_state_dict(meta)
        _runs[name] = (z, meta, CadrlModule.from_state_dict(sd).eval(), CadrlModule.from_state_dict(sd).double().eval())
    return _runs[name]


def row_error(m32, m64, rows):
    """max |value_network float32 - float64 copy| over rows [..., 13] (a float32 tensor)."""
    x = rows.reshape(-1, rows.shape[-1]).cpu()
    with torch.no_grad():
        return float((m32.value_network(x).double() - m64.value_network(x.double())).abs().max())


def chosen_index(z, t):
    return int(np.where((z["action_space"] == z["action"][t]).all(1))[0][0])
