"""OM-SARL without a GPU: ebcsim.occupancy.occupancy_maps against the reference's own build_occupancy_maps (constructed
states, and the maps its predict() built during the recorded runs), the host build of csrc/ebc_om_rule.h byte for byte
against it (also as a program of its own under AddressSanitizer and UBSan), the facade policy on the oracle backend
against the recorded runs, configuration, and the new ABI entry.  Goldens: tests/golden/make_golden_om.py; cases and
tolerances: tests/om_cases.py."""
import configparser
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi, config as ebc_config
from ebcsim.occupancy import OccupancySpec, boundary_margin, occupancy_maps, widen
from om_cases import (ENVS, GRIDS, MARGIN, REFUSALS, ROOT, ROWS, RUNS, TOL_FACTOR, chosen_index, compare_maps, edge_batch, golden_cases,
                      golden_run, golden_weights_file, host_om, host_program, om_args, read_results, shape_sweep, value_error,
                      write_batches)

HEADER = os.path.join(ROOT, "include", "ebcsim.h")
PROFILE = os.path.join(ROOT, "profiles", "om_accuracy.txt")
_accuracy = {}


@pytest.fixture(scope="module", autouse=True)
def accuracy_profile():
    """After the module's tests: profiles/om_accuracy.txt from what they measured, when everything has been measured."""
    yield
    if set(_accuracy) != {"cases"} | {("maps", n) for n in RUNS} | {("facade", n) for n in RUNS}:
        return
    out = ["# OM-SARL accuracy, written by tests/test_om_cpu.py.  Maps: ebcsim.occupancy.occupancy_maps (the algebraic frame)",
           "# against the reference's own build_occupancy_maps (arctan2 / cos / sin); occupancy columns are equal everywhere, the",
           "# figure is the largest difference of a mean-velocity column (bound: one float32 spacing + 1e-12); `closest`: the",
           "# smallest distance of a non-coincident coordinate to a cell boundary, in cells (no pair is left out below %g)." % MARGIN,
           "# Facade: e_ref = the network in torch float32 against a float64 copy on the rows the policy built; bound = %d * e_ref." % TOL_FACTOR,
           ""]
    n, diff, closest = _accuracy["cases"]
    out.append("om_cases: %d states, largest velocity difference %.3g, closest %.3g" % (n, diff, closest))
    for name in RUNS:
        n, diff, closest = _accuracy["maps", name]
        out.append("%s maps: %d decisions, largest velocity difference %.3g, closest %.3g" % (name, n, diff, closest))
    for name in RUNS:
        n, e_ref, err, gap = _accuracy["facade", name]
        out.append("%s facade: %d decisions, e_ref %.3g, |values - recorded| %.3g (bound %.3g), smallest recorded top-2 gap %.3g" % (
            name, n, e_ref, err, TOL_FACTOR * e_ref, gap))
    with open(PROFILE, "w") as f:
        f.write("\n".join(out) + "\n")


def test_maps_against_the_references_on_constructed_states():
    """Every state of om_cases.npz (all kinds, channel counts and grids): occupancy equal, mean velocities within one float32
    spacing + 1e-12, and NO non-coincident pair within MARGIN cells of a boundary (none is left out of the comparison)."""
    cases = golden_cases()
    kinds, grids, diff, closest = set(), set(), 0.0, np.inf
    for ob, spec, kind, want in cases:
        margin = float(boundary_margin(ob[None], None, spec).min())
        assert margin >= MARGIN, (kind, spec, margin)
        closest = min(closest, margin)
        diff = max(diff, compare_maps(occupancy_maps(ob[None], None, spec)[0], want, spec))
        kinds.add(kind)
        grids.add((spec.cell_num, spec.cell_size, spec.channels))
    assert kinds == {"random", "coincident", "standing", "zero_sign", "far", "two_rows"}
    assert grids == {(n, s, c) for n, s in ((4, 1.0), (3, 0.5), (5, 0.7), (8, 1.0)) for c in (1, 2, 3)}
    assert sum(k == "random" for _, _, k, _ in cases) >= 300
    _accuracy["cases"] = (len(cases), diff, closest)
    print("om_cases: %d states, largest velocity difference %.3g, closest boundary %.3g cells" % (len(cases), diff, closest))


@pytest.mark.parametrize("name", RUNS)
def test_maps_against_the_recorded_runs(name):
    """The maps the reference's predict() built at every decision of a recorded run, from the rows it built them from."""
    z, meta, spec, _, _ = golden_run(name)
    ob, want = z["om_ob"], z["om"]
    assert ob.shape[0] == want.shape[0] == len(z["action"]) and want.shape[2] == spec.width
    margin = float(boundary_margin(ob, None, spec).min())
    assert margin >= MARGIN, margin
    diff = compare_maps(occupancy_maps(ob, None, spec), want, spec)
    assert want.any(), "no cell of the run is ever occupied"
    _accuracy["maps", name] = (len(ob), diff, margin)
    print("%s: %d decisions, largest velocity difference %.3g, closest boundary %.3g cells" % (name, len(ob), diff, margin))


def test_padding_rows_and_widen():
    """Rows at or past n_valid are never read (NaN there reaches nothing) and get zero maps; n_valid = None is n_valid = R;
    widen appends an env's maps to every action's rows, numpy and torch alike."""
    ob, nv, rows, spec = edge_batch(3, 18, 2, 13, 4, 3)
    om = occupancy_maps(ob, nv, spec)
    assert np.isfinite(om).all()
    for e in range(3):
        n = max(0, min(18, int(nv[e])))
        assert (om[e, n:] == 0).all()
        if n:
            assert om[e, :n].tobytes() == occupancy_maps(ob[e:e + 1, :n], None, spec)[0].tobytes()
    wide = widen(rows, om)
    assert wide.shape == (3, 2, 18, 13 + 48) and wide.dtype == np.float32
    assert wide[..., :13].tobytes() == rows.tobytes() and all(wide[:, a, :, 13:].tobytes() == om.tobytes() for a in range(2))
    assert widen(torch.from_numpy(rows), torch.from_numpy(om)).numpy().tobytes() == wide.tobytes()
    with pytest.raises(NotImplementedError):
        OccupancySpec(4, 1.0, 4)
    with pytest.raises(ValueError):
        OccupancySpec(0, 1.0, 3)
    with pytest.raises(ValueError):
        OccupancySpec(4, float("inf"), 3)


def test_host_build_equals_numpy_bytes():
    """tests/native/om_host.cc (g++) against occupancy_maps: the same bytes on every state of om_cases.npz and on the edge
    batches of every grid (ragged n_valid with 0, 1, R; NaN past n_valid; far occupants; coincident rows; zero velocities of
    both signs), and its wide rows are widen()'s."""
    for ob, spec, kind, _ in golden_cases():
        assert host_om(ob[None], None, spec)[0].tobytes() == occupancy_maps(ob[None], None, spec).tobytes(), (kind, spec)
    for g, (cell_num, channels) in enumerate(GRIDS):
        for E, R, A, T in shape_sweep(g):
            if E * A * R > 40000:
                A = 2
            ob, nv, rows, spec = edge_batch(E, R, A, T, cell_num, channels)
            om, wide = host_om(ob, nv, spec, rows)
            want = occupancy_maps(ob, nv, spec)
            tag = "E %d R %d A %d T %d grid %s" % (E, R, A, T, (cell_num, channels))
            assert om.tobytes() == want.tobytes(), tag
            assert wide.tobytes() == widen(rows, want).tobytes(), tag
    ob, nv, rows, spec = edge_batch(3, 18, 2, 17, 4, 3)
    full = np.full((3,), 18, dtype=np.int64)
    clean = np.nan_to_num(ob, nan=0.5)
    assert host_om(clean, None, spec)[0].tobytes() == host_om(clean, full, spec)[0].tobytes()


def test_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/om_host.cc as a program of its own with -fsanitize=address,undefined on the golden states and the edge
    batches: no finding (a finding ends the program with a non-zero status), and the bytes of the library build."""
    batches = [(ob[None], None, spec, None) for ob, spec, _, _ in golden_cases()]
    for g, (cell_num, channels) in enumerate(GRIDS):
        for E, R, A, T in shape_sweep(g):
            if E * A * R > 4000:
                A = 1
            ob, nv, rows, spec = edge_batch(E, R, A, T, cell_num, channels)
            batches.append((ob, nv, spec, rows if E < 65 or R < 128 else None))
    src, dst = str(tmp_path / "edges.bin"), str(tmp_path / "out.bin")
    write_batches(src, batches)
    r = subprocess.run([host_program(sanitize=True), src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d batches" % len(batches) in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    for (ob, nv, spec, rows), (om, wide) in zip(batches, read_results(dst, batches)):
        want_om, want_wide = host_om(ob, nv, spec, rows)
        assert om.tobytes() == want_om.tobytes() and (wide is None or wide.tobytes() == want_wide.tobytes()), ob.shape
    raw = open(src, "rb").read()
    open(src, "wb").write(raw[:len(raw) - 5])
    r = subprocess.run([host_program(sanitize=True), src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "malformed" in r.stderr


def _facade(meta, tmp_path, phase="train", weights=None):
    from ebcsim.env import configure_env_policy_robot
    from oracle import oracle
    env_path, pol_path = tmp_path / "env.config", tmp_path / "policy.config"
    env_path.write_text(meta["config_text"])
    pol_path.write_text(meta["policy_config_text"])
    return configure_env_policy_robot(str(env_path), str(pol_path), weights or golden_weights_file(meta, tmp_path), phase=phase,
                                      policy="sarl", backend_factory=lambda p, E, N, S: oracle.OracleEnv(p, E, N, S))


def _abi_code(info):
    return {"Nothing": _abi.INFO_NOTHING, "Danger": _abi.INFO_DANGER, "ReachGoal": _abi.INFO_REACH_GOAL,
            "CollisionObstacle": _abi.INFO_COLLISION_OBSTACLE, "CollisionAdult": _abi.INFO_COLLISION_ADULT,
            "CollisionBicycle": _abi.INFO_COLLISION_BICYCLE, "CollisionChild": _abi.INFO_COLLISION_CHILD,
            "Timeout": _abi.INFO_TIMEOUT}[type(info).__name__]


@pytest.mark.parametrize("name", RUNS)
def test_om_sarl_facade_run(name, tmp_path):
    """configure_env_policy_robot(..., policy="sarl") with with_om = true on the oracle backend, phase "train", epsilon 0:
    the recorded action at every decision, the values within TOL_FACTOR * e_ref, last_state [R, T + W], reward and info;
    one sweep per decision."""
    z, meta, spec, n32, n64 = golden_run(name)
    env, pol, robot = _facade(meta, tmp_path)
    W = spec.width
    T = 17 if meta["with_agent_type"] else 13
    assert type(pol).__name__ == "SARL" and pol.name == "OM-SARL" and pol.with_om is True
    assert pol.input_dim() == T + W == meta["input_dim"] and pol.om_spec() == spec
    assert list(pol.get_model().state_dict()) == [k for k, _, _ in meta["state_dict"]]
    pol.set_epsilon(0.0)
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    assert len(ob) == meta["rows"]
    net, seen = pol._value_net(), []
    forward = net.action_values
    net.action_values = lambda rows, *a, **kw: (seen.append(value_error(n32, n64, rows)), forward(rows, *a, **kw))[1]
    done, t, err = False, 0, 0.0
    while not done:
        assert t < len(z["action"])
        calls = env.backend_calls
        action = robot.act(ob, env=env)
        assert env.backend_calls == calls + 1 and len(seen) == t + 1  # one sweep per decision
        np.testing.assert_allclose([action[0], action[1]], z["action"][t], atol=1e-12, err_msg="decision %d" % t)
        err = max(err, float(np.abs(np.array(pol.action_values) - z["values"][t]).max()))
        last = pol.last_state.numpy()
        assert last.shape == (meta["rows"], T + W) and last.dtype == np.float32
        np.testing.assert_allclose(last[:, :T], z["last_state"][t][:, :T], atol=1e-5, rtol=1e-5, err_msg="decision %d" % t)
        compare_maps(last[:, T:], z["last_state"][t][:, T:], spec)
        assert pol.get_attention_weights().shape == (meta["rows"],)
        ob, _, reward, done, info = env.step(action, compute_local_map=False)
        np.testing.assert_allclose(reward, z["reward"][t], atol=1e-9)
        assert _abi_code(info) == int(z["info"][t]), t
        t += 1
    assert t == len(z["action"]) and _abi_code(info) == int(meta["final_info"])
    top = np.sort(z["values"], axis=1)
    gap = float((top[:, -1] - top[:, -2]).min())
    _accuracy["facade", name] = (t, max(seen), err, gap)
    print("%s: %d decisions, e_ref %.3g, |values - recorded| %.3g (bound %.3g), gap %.3g" % (name, t, max(seen), err, TOL_FACTOR * max(seen), gap))
    assert err <= TOL_FACTOR * max(seen), (err, max(seen))


def _policy_cfg(meta, **sarl):
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["policy_config_text"])
    for k, v in sarl.items():
        cfg.set("sarl", k, v)
    return cfg


def test_configure_with_om():
    """with_om = true: input_dim() = T + cell_num^2 * om_channel_size (multi_human_rl.py:151-154), name "OM-SARL", mlp1 that
    wide; with_om = false: today's SARL."""
    from ebcsim.rl_policy import SARL
    for name in RUNS:
        _, meta, spec, _, _ = golden_run(name)
        T = 17 if meta["with_agent_type"] else 13
        pol = SARL()
        pol.configure(_policy_cfg(meta))
        assert pol.with_om is True and pol.name == "OM-SARL" and pol.input_dim() == T + spec.width == meta["input_dim"]
        assert pol.get_model().state_dict()["mlp1.0.weight"].shape[1] == T + spec.width
        assert OccupancySpec.from_config(_policy_cfg(meta)) == spec
        assert ebc_config.occupancy_from_config(_policy_cfg(meta)) == spec
        assert ebc_config.occupancy_from_config(_policy_cfg(meta), policy="cadrl") is None
        plain = SARL()
        plain.configure(_policy_cfg(meta, with_om="false"))
        assert plain.with_om is False and plain.name == "SARL" and plain.input_dim() == T and plain.om_spec() is None
        assert OccupancySpec.from_config(_policy_cfg(meta, with_om="false")) is None


def test_wrong_width_one_row_state_and_lstm(tmp_path):
    """A network of another width is a ValueError (facade and DeviceSarlPolicy's check); a one-row state raises the
    reference's ValueError (np.concatenate of nothing, multi_human_rl.py:164); LstmRL still refuses with_om."""
    from ebcsim.rl_policy import SARL, LstmRL
    from ebcsim.state import ObservableState
    _, meta, spec, n32, _ = golden_run(RUNS[0])
    env, pol, robot = _facade(meta, tmp_path)
    pol.set_epsilon(0.0)
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    plain = SARL()
    plain.configure(_policy_cfg(meta, with_om="false"))
    pol.model = plain.get_model()  # 13 wide
    pol._net = None
    with pytest.raises(ValueError, match="wide"):
        robot.act(ob, env=env)
    om_pol = SARL()
    om_pol.configure(_policy_cfg(meta))
    with pytest.raises(ValueError, match="concatenate"):
        om_pol.build_occupancy_maps([ObservableState(0.0, 0.0, 0.1, 0.0, 0.3)])
    assert tuple(om_pol.build_occupancy_maps([ObservableState(0.0, 0.0, 0.1, 0.0, 0.3), ObservableState(0.4, 0.0, 0.0, 0.0, 0.3)]).shape) == (2, spec.width)
    cfg = _policy_cfg(meta)
    cfg.set("lstm_rl", "with_om", "true")
    with pytest.raises(NotImplementedError):
        LstmRL().configure(cfg)


def test_om_entry_in_header_and_bindings(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+ebc_occupancy_rows\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 3 == len(_capi.SYMBOLS["ebc_occupancy_rows"][1])
    assert _capi.SYMBOLS["ebc_occupancy_rows"][0] is C.c_int
    assert "#define EBC_ABI_VERSION 1" in text and _abi.ABI_VERSION == 1
    fields = [f[0] for f in _abi.EbcOmArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",sizeof(EbcOmArgs));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu",offsetof(EbcOmArgs,%s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
    A = _abi.EbcOmArgs
    assert sizes == [C.sizeof(A)] + [getattr(A, f).offset for f in fields]
    assert fields[0] == "struct_size"


def test_om_entry_validates_its_arguments():
    """What can be refused without a device is refused before one is touched, with the reason in ebc_last_error."""
    lib = _capi.lib()
    for kw, reason in REFUSALS:
        a = om_args(**kw)
        assert lib.ebc_occupancy_rows(0, None, C.addressof(a)) == _abi.ERR_UNSUPPORTED, kw
        assert reason in lib.ebc_last_error(), (kw, lib.ebc_last_error())
    a = om_args(size=8)
    assert lib.ebc_occupancy_rows(0, None, C.addressof(a)) == _abi.ERR_INVALID and b"struct_size" in lib.ebc_last_error()
    for kw in (dict(next_ob=None), dict(E=-1), dict(R=0)):
        a = om_args(**kw)
        assert lib.ebc_occupancy_rows(0, None, C.addressof(a)) == _abi.ERR_INVALID, kw
    assert lib.ebc_occupancy_rows(0, None, None) == _abi.ERR_INVALID


@pytest.mark.parametrize("tool", ["om_bench.py", "evaluate.py"])
def test_om_tools_parse_and_show_their_usage(tool, tmp_path):
    import py_compile
    import sys
    path = os.path.join(ROOT, "tools", tool)
    py_compile.compile(path, cfile=str(tmp_path / (tool + "c")), doraise=True)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    if tool == "evaluate.py":
        _, meta, _, _, _ = golden_run(RUNS[0])
        pol_path = tmp_path / "policy.config"
        pol_path.write_text(meta["policy_config_text"])
        r = subprocess.run([sys.executable, path, "--policy", "sarl", "--policy-config", str(pol_path)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--weights" in r.stderr and "with_om" in r.stderr
