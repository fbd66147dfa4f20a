"""Shared by tests/test_om_lstm_cpu.py and tests/test_om_lstm_gpu.py: the golden OM-LSTM runs (tests/golden/om_lstm_*.npz:
the reference's own LstmRL with with_om = true), the constructed states of the sorted wide state (ties, NaN keys, the
order-sensitivity scene), the 61- and 64-wide networks of the gradient, and the accuracy table both the GPU test and
profiles/om_lstm_grad_accuracy.txt come from.

Tolerances.  Values: F_CELL (tests/lstm_cases.py) x the error of LstmModule in float32 against a float64 copy of it on the
same rows, measured by the tests.  last_state: the first 13 columns at the rotate tolerance of tests/test_lstm_cpu.py
(1e-5 absolute and relative), the maps by om_cases.compare_maps.  Gradient: per parameter tensor err = max |g - g_64| /
max |g_64| against float64 autograd of LstmModule on the same float32 weights and inputs, within TOL_FACTOR (8) x torch's own
float32 error, floored at YARDSTICK_FLOOR = 2^-25 (tests/lstm_grad_cases.py).  Each seeded batch is taken as its seed gives
it; the floor stands in for the search for a usable seed."""
import json
import os

import numpy as np
import torch

import lstm_grad_cases as lg
from lstm_cases import F_CELL, tensor_digest  # noqa: F401
from lstm_grad_cases import TOL_FACTOR, YARDSTICK_FLOOR  # noqa: F401
from ebcsim.occupancy import OccupancySpec
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ["om_lstm_interaction_a5", "om_lstm_interaction_n10", "om_lstm_plain_a5", "om_lstm_plain_n10"]
ROTATE_TOL = 1e-5
OM = OccupancySpec(4, 1.0, 3)  # the reference's [om]: 13 + 48 = 61 columns
WIDTHS = [61, 64]  # the reference's own width and the kernels' limit (EBC_LSTM_MAX_DIM, EBC_LSTM_GRAD_MAX_IN)


def wide(net, T):
    """A network of tests/lstm_grad_cases.py with rows T wide."""
    widths, S, two = net
    return ([T] + list(widths[1:]), S, two)


# narrow and reference widths, with and without mlp1, at both row widths
GRAD_NETS = [wide(net, T) for T in WIDTHS for net in (lg.NARROW_NET2, lg.NARROW_NET1, lg.REFERENCE_NET2, lg.REFERENCE_NET1)]
GRAD_IDS = ["%d_%s_%s" % (n[0][0], "narrow" if n[0][5] == 7 else "reference", "mlp1" if n[2] else "plain") for n in GRAD_NETS]
# lstm_grad_lds_floats at the reference widths with 61 columns: what ebc_lstm_net_grad_max_rows returns there
REFERENCE_MAX_ROWS = {True: 11, False: 23}


# ---------------------------------------------------------------------- the golden runs
def golden_state_dict(meta):
    """The network of a golden run, as its generator made it: LstmModule of the run's policy config with rows
    meta["input_dim"] wide, built after torch.manual_seed(meta["torch_seed"]), every tensor held to the name, shape and
    SHA-256 recorded from the reference's own get_model().state_dict()."""
    import configparser
    from ebcsim.lstm_rl import LstmModule
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["policy_config_text"])
    dims = lambda key: [int(x) for x in cfg.get("lstm_rl", key).split(", ")]  # noqa: E731
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(meta["torch_seed"]))
        m = LstmModule(int(meta["input_dim"]), 6, dims("mlp2_dims"), cfg.getint("lstm_rl", "global_state_dim"),
                       dims("mlp1_dims") if cfg.getboolean("lstm_rl", "with_interaction_module") else None)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    want = meta["state_dict"]
    assert list(sd) == [k for k, _, _ in want], (list(sd), [k for k, _, _ in want])
    for k, shape, digest in want:
        assert list(sd[k].shape) == shape and sd[k].dtype == torch.float32, k
        assert tensor_digest(sd[k]) == digest, "%s: this torch does not rebuild the recorded tensor from seed %d" % (k, meta["torch_seed"])
    return sd


def golden_weights_file(meta, directory):
    path = os.path.join(str(directory), "rl_model.bin")
    torch.save(golden_state_dict(meta), path)
    return path


_runs = {}


def golden_run(name):
    """(z, meta, spec, LstmModule float32, its float64 copy) of a golden run, built once."""
    if name not in _runs:
        from ebcsim.lstm_rl import LstmModule
        z = load(name)
        meta = json.loads(str(z["meta"]))
        sd = golden_state_dict(meta)
        spec = OccupancySpec(meta["cell_num"], meta["cell_size"], meta["channels"])
        m32 = LstmModule.from_state_dict(sd).eval()
        assert m32.with_interaction_module == bool(meta["with_interaction_module"]) and m32.input_dim == 13 + spec.width == 61
        _runs[name] = (z, meta, spec, m32, LstmModule.from_state_dict(sd).double().eval())
    return _runs[name]


def value_error(m32, m64, rows):
    """max |LstmModule float32 - its float64 copy| over the joint states rows [..., R, 61] (a float32 tensor)."""
    x = rows.reshape(-1, rows.shape[-2], rows.shape[-1]).cpu()
    with torch.no_grad():
        return float((m32(x).double() - m64(x.double())).abs().max())


def chosen_index(z, t):
    return int(np.where((z["action_space"] == z["action"][t]).all(1))[0][0])


# ---------------------------------------------------------------------- constructed states
# The robot stands at the origin and heads for (0, 4).  (px, py, vx, vy) of the rows in the env's order.
BIG = float(2 ** 60)
# Row 3 moves with (1, 0): its frame is the world's.  Rows 0, 1, 2 fall into cell (2, 2) of its 4 x 4 map (k = 10) with
# vx = 2^60, 1, -2^60.  By distance to the robot they sort 0, 2, 1, 3: the cell's float64 sum is (2^60 - 2^60) + 1 = 1 in the
# sorted order (mean 1 / 3) and (2^60 + 1) - 2^60 = 0 in the env's.
ORDER_SCENE = np.array([[2.6, 0.5, BIG, 0.0], [2.4, 0.5, 1.0, 0.0], [2.5, 0.5, -BIG, 0.0], [2.0, 0.0, 1.0, 0.0]])
ORDER_SORTED = [0, 2, 1, 3]
ORDER_CELL = 10
# Rows 0 and 1 mirror each other about the robot's heading: the same float32 distance, they keep the env's order behind row 2
MIRROR_SCENE = np.array([[1.5, 1.0, 0.1, 0.0], [-1.5, 1.0, -0.1, 0.0], [0.5, 3.0, 0.0, 0.2]])
MIRROR_SORTED = [2, 0, 1]
ROBOT = [0.0, 0.0, 0.0, 0.0, 0.3, 0.0, 4.0, 1.0, np.pi / 2]
RADIUS = 0.3


def scene_batch(rows_list, N=4, S=0):
    """One env per entry of rows_list ([n, 4] arrays: humans, n <= N), the robot of ROBOT, ebcsim.scene.SceneBatch."""
    from ebcsim import scene as ebc_scene
    E = len(rows_list)
    f = lambda *s: np.zeros(s)  # noqa: E731
    nh = np.array([len(r) for r in rows_list], np.int32)
    b = ebc_scene.SceneBatch(E, N, S, nh, f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                             np.zeros((E, N), np.uint8), np.zeros(E, np.int32), f(E, max(S, 1)), f(E, max(S, 1)), f(E, max(S, 1)), None, f(E, 9))
    for e, rows in enumerate(rows_list):
        n = len(rows)
        b.px[e, :n], b.py[e, :n], b.vx[e, :n], b.vy[e, :n] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
        b.gx[e, :n], b.gy[e, :n] = -rows[:, 0], -rows[:, 1]
        b.radius[e, :n], b.v_pref[e, :n] = RADIUS, 1.0
        b.robot[e] = ROBOT
    return b


def rotated_of(rows):
    """The rotated rows [n, 13] float32 of a constructed state by the policy object's rotate(): the robot of ROBOT."""
    from ebcsim.rl_policy import LstmRL
    pol = LstmRL()
    pol.kinematics = "holonomic"
    full = torch.tensor([ROBOT + [float(r[0]), float(r[1]), float(r[2]), float(r[3]), RADIUS] for r in rows], dtype=torch.float32)
    return pol.rotate(full).numpy().astype(np.float32)


def ob_of(rows):
    """[n, 5] float64 (px, py, vx, vy, radius) of a constructed state."""
    return np.concatenate([np.asarray(rows, dtype=np.float64), np.full((len(rows), 1), RADIUS)], axis=1)


def order_cell_means(wide_row, spec=OM, T=13):
    """(occupied, mean vx, mean vy) of cell ORDER_CELL in one wide row."""
    at = T + ORDER_CELL * spec.channels
    return tuple(float(x) for x in wide_row[at:at + 3])


# ---------------------------------------------------------------------- the gradient on wide rows
def accuracy_cases():
    """("golden", run): the run's stored states with the recorded values of the chosen actions as targets; ("seeded", net
    index into GRAD_NETS, B, R, gate scale)."""
    c = lg.chunk()
    return ([("golden", name) for name in RUNS]
            + [("seeded", ni, 2 * c + 1, 5, s) for ni in (0, 1, 4, 5) for s in lg.SCALES]
            + [("seeded", ni, 100, 10, s) for ni in (2, 3) for s in lg.SCALES]
            + [("seeded", ni, c + 1, 5, 1.0) for ni in (6, 7)])


def kernel_accuracy_cases():
    """accuracy_cases() that ebc_lstm_grad takes: all but om_lstm_interaction_n10, whose 18 rows are more than the 11 a
    chunk's LDS holds for ValueNetwork2 at 61 columns (the trainer's native=False serves such a scene); that run's states
    hold the rule through the host build."""
    return [c for c in accuracy_cases() if c != ("golden", "om_lstm_interaction_n10")]


_refs, _rows, _golden = {}, {}, {}


def golden_rows(name):
    if name not in _golden:
        z, meta, _, _, _ = golden_run(name)
        idx = [chosen_index(z, t) for t in range(len(z["action"]))]
        _golden[name] = (golden_state_dict(meta), np.ascontiguousarray(z["last_state"], dtype=np.float32),
                         np.array([z["values"][t, i] for t, i in enumerate(idx)], dtype=np.float32))
    return _golden[name]


def reference_of(case):
    """The batch of a case and what the code under test has no part in: float64 and float32 autograd of LstmModule, torch's
    float32 error per tensor and of the loss.  Computed once."""
    if case not in _refs:
        if case[0] == "golden":
            sd, rows, target = golden_rows(case[1])
        else:
            _, ni, B, R, s = case
            sd = lg.random_state_dict(GRAD_NETS[ni], seed=5, scale=s)
            rows, target = lg.plain_batch(GRAD_NETS[ni], B, R, seed=930000 + 1000 * ni + 10 * B + R)
        B = rows.shape[0]
        live, scale = np.ones(B, dtype=bool), 2.0 / B
        g64, l64, _ = lg.torch_grad(sd, rows, target, None, live, scale, torch.float64)
        g32, l32, _ = lg.torch_grad(sd, rows, target, None, live, scale, torch.float32)
        _refs[case] = dict(net=lg.net_of(sd), sd=sd, rows=rows, target=target, scale=scale, g64=g64, l64=l64,
                           err32={k: lg._err(g32[k], g64[k]) for k in g64}, loss32=abs(l32 - l64) / l64)
    return _refs[case]


def accuracy_of(case, grad, loss):
    """([(tensor, err, err_torch32, bar)], the loss's likewise) of a packed gradient and loss_sum computed for the case."""
    ref = reference_of(case)
    got = lg.unpacked(ref["net"], grad)
    bar = lambda e: TOL_FACTOR * max(e, YARDSTICK_FLOOR)  # noqa: E731
    return ([(k, lg._err(got[k], ref["g64"][k]), ref["err32"][k], bar(ref["err32"][k])) for k in ref["g64"]],
            (abs(loss - ref["l64"]) / ref["l64"], ref["loss32"], bar(ref["loss32"])))


def accuracy_row(case):
    """accuracy_of the host build's result; computed once."""
    if case not in _rows:
        ref = reference_of(case)
        g, loss, count, _, _ = lg.host_grad(lg.host_pack(ref["sd"]), ref["net"], ref["rows"], ref["target"], grad_scale=ref["scale"])
        assert count == ref["rows"].shape[0]
        _rows[case] = accuracy_of(case, g, loss)
    return _rows[case]


def case_name(case):
    if case[0] == "golden":
        return case[1]
    return "net %d B %d R %d scale %g" % case[1:]


def accuracy_table():
    lines = ["LSTM-RL gradient rule on the wide rows of OM-LSTM (csrc/ebc_lstm_grad_rule.h, host build tests/native/lstm_grad_host.cc:",
             "the kernel's bytes, tests/test_om_lstm_gpu.py) against torch autograd of LstmModule in float64, beside torch's own float32",
             "autograd: err = max |g - g_64| / max |g_64| per parameter tensor.  The golden OM-LSTM runs' stored states (61 wide) with",
             "their recorded values as targets, and seeded networks and batches of tests/om_lstm_cases.py at gate scales 1 and 4, each",
             "taken as its seed gives it; bar: rule <= %d x max(torch32, 2^-25), the floor profiles/lstm_grad_accuracy.txt set;" % TOL_FACTOR,
             "`floor` marks a row whose torch32 error is below 2^-25 (the ratio printed is against torch's error all the same).", ""]
    for i, net in enumerate(GRAD_NETS):
        lines.append("net %d: %s%s" % (i, "-".join(str(w) for w in net[0]), "" if net[2] else " (no mlp1)"))
    lines += ["", "%-34s %-22s %11s %11s %7s" % ("case", "tensor", "err_rule", "err_torch32", "ratio")]
    ratio = lambda a, b: a / b if b else (float("inf") if a else 0.0)  # noqa: E731
    for case in accuracy_cases():
        tensors, (lr, lt, _) = accuracy_row(case)
        for key, er, et, _ in tensors + [("loss_sum", lr, lt, 0.0)]:
            lines.append("%-34s %-22s %11.3e %11.3e %7.2f%s" % (case_name(case), key, er, et, ratio(er, et), "  floor" if et < YARDSTICK_FLOOR else ""))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "profiles", "om_lstm_grad_accuracy.txt"), "w") as f:
        f.write(accuracy_table())
