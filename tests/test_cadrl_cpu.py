"""CADRL without a GPU: the torch network on the reference's golden runs, the facade policy, the reference's refusals,
the host build of the decision rule against a plain torch restatement on the edge batches (also as a program of its own
under AddressSanitizer and UBSan), and the new ABI entry.  Golden: the reference's own CADRL (rl/policy/cadrl.py,
torch.manual_seed(11) weights) driving full episodes with 81 action values per decision (tests/golden/cadrl_*.npz,
tests/golden/make_golden_cadrl.py)."""
import configparser
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cadrl_cases import (ACTIONS, ENVS, KINDS, ROOT, ROWS, RUNS, TOL_FACTOR, all_edge_batches, chosen_index, golden_run,
                         golden_state_dict, golden_weights_file, host_decide, host_program, read_results, restated, row_error,
                         same_values, write_batches)
from ebcsim import _abi, _capi, config as ebc_config
from helpers import batch_from_init, params_of

HEADER = os.path.join(ROOT, "include", "ebcsim.h")
PROFILE = os.path.join(ROOT, "profiles", "cadrl_accuracy.txt")
_accuracy = {}


@pytest.fixture(scope="module", autouse=True)
def accuracy_profile():
    """After the module's tests: profiles/cadrl_accuracy.txt from what they measured, when every run has been measured."""
    yield
    if len(_accuracy) != len(RUNS):
        return
    out = ["# CADRL accuracy, written by tests/test_cadrl_cpu.py.  e_ref: value_network in torch float32 against a float64 copy",
           "# of the same module, max over every row of the run's look-ahead rows (oracle env); |values - recorded| against the",
           "# reference's own recorded action values; bound = %d * e_ref; gap: the run's smallest recorded top-2 gap (the" % TOL_FACTOR,
           "# generator asserts gap > 2 * bound on the reference's own rows).", ""]
    for name in RUNS:
        n, rows, e_ref, err, gap = _accuracy[name]
        out.append("%s: %d decisions, %d rows, e_ref %.3g, |values - recorded| %.3g (bound %.3g), gap %.3g" % (
            name, n, rows, e_ref, err, TOL_FACTOR * e_ref, gap))
    with open(PROFILE, "w") as f:
        f.write("\n".join(out) + "\n")


@pytest.mark.parametrize("name", RUNS)
def test_weights_rebuild_and_load_strictly(name):
    """The seed rebuilds every recorded tensor (name, shape, SHA-256), and the reference's keys load with strict=True."""
    from ebcsim.cadrl import CadrlModule
    z, meta, m32, _ = golden_run(name)
    sd = golden_state_dict(meta)
    assert list(sd) == ["value_network.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")]
    m = CadrlModule.from_state_dict(sd)
    assert m.input_dim == 13 and [l.out_features for l in m.value_network if isinstance(l, torch.nn.Linear)] == [150, 100, 100, 1]
    assert CadrlModule(13, [150, 100, 100, 1]).load_state_dict(sd, strict=True).missing_keys == []
    with pytest.raises(RuntimeError):
        CadrlModule(13, [150, 100, 1]).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("name", RUNS)
def test_cadrl_values_cpu(name):
    """CadrlValueNet (torch, CPU) on the oracle's look-ahead rows: every recorded value within TOL_FACTOR * e_ref, the
    recorded action at every decision (the net's own choice and the reference rule on its values), the recorded reward
    and info at every step, and cadrl_one's recorded last_state."""
    from ebcsim.cadrl import CadrlValueNet
    from ebcsim.sarl import reference_choice
    from oracle import oracle
    z, meta, m32, m64 = golden_run(name)
    params = params_of(z)
    assert params.with_agent_type == 0
    b = batch_from_init(z)
    env = oracle.OracleEnv(params, 1, b.N, b.S)
    env.reset(b)
    net = CadrlValueNet(golden_state_dict(meta))
    assert net.device.type == "cpu" and net.values_decidable is False
    discount = meta["gamma"] ** (params.time_step * float(b.robot[0, 7]))
    e_ref = err = 0.0
    T = len(z["action"])
    for t in range(T):
        if "last_state" in z.files:
            np.testing.assert_allclose(env.observe()[1][0, 0], z["last_state"][t], atol=1e-5, rtol=1e-5, err_msg="decision %d" % t)
        la = env.lookahead(z["action_space"], human_policy=_abi.HUMAN_ORCA)
        rows = torch.from_numpy(la["rows_rotated"])
        assert rows.shape[2] == meta["rows"]
        e_ref = max(e_ref, row_error(m32, m64, rows))
        values = net.action_values(rows, torch.from_numpy(la["reward"]), discount)
        assert values.dtype == torch.float64 and tuple(values.shape) == (1, 81)
        err = max(err, float(np.abs(values[0].numpy() - z["values"][t]).max()))
        want = chosen_index(z, t)
        assert int(net.last_choice[0]) == want == int(reference_choice(values)[0]), t
        out = env.step(robot_action=z["action"][t][None], human_policy=_abi.HUMAN_CACHED)
        assert int(out["info"][0]) == int(z["info"][t]), t
        np.testing.assert_allclose(out["reward"][0], z["reward"][t], atol=1e-9)
    top = np.sort(z["values"], axis=1)
    gap = float((top[:, -1] - top[:, -2]).min())
    print("%s: %d decisions, e_ref %.3g, |values - recorded| %.3g (bound %.3g), gap %.3g" % (name, T, e_ref, err, TOL_FACTOR * e_ref, gap))
    _accuracy[name] = (T, meta["rows"], e_ref, err, gap)
    assert err <= TOL_FACTOR * e_ref, (err, e_ref)
    assert gap > 2 * TOL_FACTOR * e_ref, "a decision of this run lies inside the tolerance"
    assert bool(out["done"][0]) and int(out["info"][0]) == int(meta["final_info"]) == 7


def _facade(meta, tmp_path, phase, weights=None):
    from ebcsim.env import configure_env_policy_robot
    from oracle import oracle
    env_path, pol_path = tmp_path / "env.config", tmp_path / "policy.config"
    env_path.write_text(meta["config_text"])
    pol_path.write_text(meta["policy_config_text"])
    return configure_env_policy_robot(str(env_path), str(pol_path), weights or golden_weights_file(meta, tmp_path), phase=phase,
                                      policy="cadrl", backend_factory=lambda p, E, N, S: oracle.OracleEnv(p, E, N, S))


def _abi_code(info):
    return {"Nothing": _abi.INFO_NOTHING, "Danger": _abi.INFO_DANGER, "ReachGoal": _abi.INFO_REACH_GOAL,
            "CollisionObstacle": _abi.INFO_COLLISION_OBSTACLE, "CollisionAdult": _abi.INFO_COLLISION_ADULT,
            "CollisionBicycle": _abi.INFO_COLLISION_BICYCLE, "CollisionChild": _abi.INFO_COLLISION_CHILD,
            "Timeout": _abi.INFO_TIMEOUT}[type(info).__name__]


@pytest.mark.parametrize("name", RUNS)
def test_cadrl_facade_run(name, tmp_path):
    """configure_env_policy_robot(..., policy="cadrl") in the run's own phase: the recorded action, values, reward and
    info at every step, one sweep and one forward per decision, and cadrl_one's last_state [13]."""
    z, meta, m32, m64 = golden_run(name)
    env, pol, robot = _facade(meta, tmp_path, meta["phase"])
    assert type(pol).__name__ == "CADRL" and pol.name == "CADRL" and pol.trainable and pol.multiagent_training is False
    assert pol.with_agent_type is False and pol.joint_state_dim == 13 and pol.gamma == 0.9 and pol.query_env is True
    assert list(pol.get_model().state_dict()) == [k for k, _, _ in meta["state_dict"]]
    pol.set_epsilon(0.0)
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    assert len(ob) == meta["rows"]
    net, seen = pol._value_net(), []
    forward = net.action_values
    net.action_values = lambda rows, *a, **kw: (seen.append(row_error(m32, m64, rows)), forward(rows, *a, **kw))[1]
    done, t, err = False, 0, 0.0
    while not done:
        assert t < len(z["action"])
        calls = env.backend_calls
        action = robot.act(ob, env=env)
        assert env.backend_calls == calls + 1 and len(seen) == t + 1 and pol._value_net() is net and net.native_forwards == 0
        np.testing.assert_allclose([action[0], action[1]], z["action"][t], atol=1e-12, err_msg="decision %d" % t)
        err = max(err, float(np.abs(np.array(pol.action_values) - z["values"][t]).max()))
        if meta["phase"] == "train":
            last = pol.last_state.numpy()
            assert last.shape == (13,) and last.dtype == np.float32
            np.testing.assert_allclose(last, z["last_state"][t], atol=1e-5, rtol=1e-5, err_msg="decision %d" % t)
        ob, _, reward, done, info = env.step(action, compute_local_map=False)
        np.testing.assert_allclose(reward, z["reward"][t], atol=1e-9)
        assert _abi_code(info) == int(z["info"][t]), t
        t += 1
    assert t == len(z["action"]) and _abi_code(info) == int(meta["final_info"])
    assert err <= TOL_FACTOR * max(seen), (err, max(seen))  # e_ref on the rows the policy itself built


def test_cadrl_keeps_the_references_refusals(tmp_path):
    """Phase "train" with five humans ends in transform()'s AssertionError (cadrl.py:231); a network whose every value
    is NaN leaves max_action None (cadrl.py:193), not a ValueError; rows of another width are refused by name."""
    z, meta, _, _ = golden_run("cadrl_a5")
    env, pol, robot = _facade(meta, tmp_path, "train")
    pol.set_epsilon(0.0)
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    assert len(ob) == 5
    with pytest.raises(AssertionError):
        robot.act(ob, env=env)
    sd = golden_state_dict(meta)
    sd["value_network.6.bias"] = torch.full_like(sd["value_network.6.bias"], float("nan"))
    path = str(tmp_path / "nan_model.bin")
    torch.save(sd, path)
    env, pol, robot = _facade(meta, tmp_path, "test", weights=path)
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    assert robot.act(ob, env=env) is None
    assert len(pol.action_values) == 81 and np.isnan(pol.action_values).all()
    from ebcsim.cadrl import CadrlValueNet
    with pytest.raises(ValueError):
        CadrlValueNet(golden_state_dict(meta)).forward(torch.zeros((2, 3, 17)))


def test_module_minimum_is_torch_min_over_the_rows_that_exist():
    """CadrlModule.forward: NaN in a valid row makes the minimum NaN, padding rows (NaN, -inf) never enter, no row gives
    NaN; the network row by row and torch.min, state by state."""
    from ebcsim.cadrl import CadrlModule, min_over_rows, running_choice
    _, meta, m32, _ = golden_run("cadrl_a5")
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(6, 4, 13, generator=g)
    nv = torch.tensor([4, 2, 0, 1, 3, 4])
    rows[1, 2:] = float("nan")
    rows[3, 1:] = float("-inf")
    rows[4, 1] = float("nan")  # a valid row
    with torch.no_grad():
        got = m32(rows, nv)
        full = m32(rows[[0, 5]])
    for b in range(6):
        n = int(nv[b])
        with torch.no_grad():
            want = torch.min(m32.value_network(rows[b, :n]), 0)[0][0] if n else torch.tensor(float("nan"))
        assert torch.allclose(got[b], want, rtol=0, atol=1e-6, equal_nan=True), b  # torch's GEMM rounds a batch of 24 rows its own way
    assert torch.isnan(got[2]) and torch.isnan(got[4]) and torch.isfinite(got[[0, 1, 3, 5]]).all()
    assert torch.allclose(full, got[[0, 5]], rtol=0, atol=1e-6)
    v = torch.tensor([[1.0, float("nan")], [float("nan"), float("nan")]])
    assert torch.isnan(min_over_rows(v)).all()
    vals = torch.tensor([[float("nan"), 2.0, 2.0, 1.0], [float("nan"), float("-inf"), float("nan"), float("-inf")],
                         [float("-inf"), float("inf"), float("inf"), 0.0]], dtype=torch.float64)
    assert running_choice(vals).tolist() == [1, -1, 1]


@pytest.mark.parametrize("A", ACTIONS)
def test_host_rule_against_the_restatement(A):
    """The g++ build of ebc_cadrl_rule.h against torch.min and the reference's running choice on every edge batch of
    this action count: the same values (NaN where NaN), the same choice."""
    seen = set()
    for E in ENVS:
        for R in ROWS:
            v, nv, reward, discount, kinds = all_edge_batches()[E, A, R]
            values, choice = host_decide(v, nv, reward, discount)
            want_values, want_choice = restated(v, nv, reward, discount)
            tag = "E %d A %d R %d" % (E, A, R)
            assert same_values(values, want_values), tag
            np.testing.assert_array_equal(choice, want_choice, err_msg=tag)
            seen.update(kinds)
            for e, kind in enumerate(kinds):
                if kind in ("all_nan", "no_rows"):
                    assert choice[e] == -1 and np.isnan(values[e]).all(), (tag, e, kind)
                elif kind in ("tie_halves", "tie_inside") and A > 1:
                    tied = np.nonzero(values[e] == values[e].max())[0]
                    assert len(tied) == 2 and choice[e] == tied[0], (tag, e, kind)
                    if kind == "tie_halves" and A > 64:
                        assert tied[1] == tied[0] + 64
                elif kind in ("full", "ragged"):
                    assert np.isfinite(values[e]).all() and choice[e] == int(np.argmax(values[e])), (tag, e, kind)
            if E > 1:  # n_valid = NULL is n_valid = R
                full = np.full((E,), R, dtype=np.int64)
                a, b = host_decide(v, None, reward, discount), host_decide(v, full, reward, discount)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), tag
    assert seen == set(KINDS)


def test_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/cadrl_host.cc as a program of its own with -fsanitize=address,undefined on every edge batch: no
    finding (a finding ends the program with a non-zero status), and the bytes of the library build."""
    batches = [(v, nv, reward, discount) for (v, nv, reward, discount, _) in all_edge_batches().values()]
    batches += [(b[0], None, b[2], b[3]) for b in batches[:6]]
    src, dst = str(tmp_path / "edges.bin"), str(tmp_path / "out.bin")
    write_batches(src, batches)
    r = subprocess.run([host_program(sanitize=True), src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d batches" % len(batches) in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    for (v, nv, reward, discount), (values, choice) in zip(batches, read_results(dst, batches)):
        want_values, want_choice = host_decide(v, nv, reward, discount)
        assert values.tobytes() == want_values.tobytes() and choice.tobytes() == want_choice.tobytes(), v.shape
    # a truncated file is refused, not read past its end
    raw = open(src, "rb").read()
    open(src, "wb").write(raw[:len(raw) - 5])
    r = subprocess.run([host_program(sanitize=True), src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "malformed" in r.stderr


def test_cadrl_entry_in_header_and_bindings(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+ebc_cadrl_decide\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 2 == len(_capi.SYMBOLS["ebc_cadrl_decide"][1])
    assert _capi.SYMBOLS["ebc_cadrl_decide"][0] is C.c_int
    assert "#define EBC_ABI_VERSION 1" in text and _abi.ABI_VERSION == 1
    fields = [f[0] for f in _abi.EbcCadrlArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",sizeof(EbcCadrlArgs));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu",offsetof(EbcCadrlArgs,%s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
    A = _abi.EbcCadrlArgs
    assert sizes == [C.sizeof(A)] + [getattr(A, f).offset for f in fields]
    assert fields[0] == "struct_size"


def test_cadrl_entry_validates_its_arguments():
    """What can be refused without a device is refused before one is touched, with the reason in ebc_last_error."""
    lib = _capi.lib()
    buf = np.zeros(8, dtype=np.float64).ctypes.data

    def call(E=1, A=1, R=1, size=None, **ptrs):
        a = _abi.EbcCadrlArgs()
        a.struct_size = C.sizeof(a) if size is None else size
        a.E, a.A, a.R, a.discount = E, A, R, 0.9
        for k in ("v", "reward", "values", "choice"):
            setattr(a, k, ptrs.get(k, buf))
        return lib.ebc_cadrl_decide(None, C.addressof(a))
    assert call(A=129) == _abi.ERR_UNSUPPORTED and b"A > 128" in lib.ebc_last_error()
    assert call(R=129) == _abi.ERR_UNSUPPORTED and b"R > 128" in lib.ebc_last_error()
    assert call(A=0) == _abi.ERR_UNSUPPORTED and b"A < 1" in lib.ebc_last_error()
    assert call(R=0) == _abi.ERR_UNSUPPORTED and b"R < 1" in lib.ebc_last_error()
    assert call(size=8) == _abi.ERR_INVALID and b"struct_size" in lib.ebc_last_error()
    assert call(v=None) == _abi.ERR_INVALID and call(choice=None) == _abi.ERR_INVALID and call(E=-1) == _abi.ERR_INVALID
    assert lib.ebc_cadrl_decide(None, None) == _abi.ERR_INVALID


def test_params_from_config_takes_cadrl():
    path = os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config")
    pol = ebc_config.read_config(path)
    assert pol.getboolean("sarl", "with_agent_type")
    _, meta, _, _ = golden_run(RUNS[0])
    env_cfg = configparser.RawConfigParser()
    env_cfg.read_string(meta["config_text"])
    default = ebc_config.params_from_config(env_cfg, pol)
    assert default.with_agent_type == 1
    cadrl = ebc_config.params_from_config(env_cfg, pol, policy="cadrl")
    assert cadrl.with_agent_type == 0
    d, e = ebc_config.params_to_dict(default), ebc_config.params_to_dict(cadrl)
    assert {k for k in d if json.dumps(d[k]) != json.dumps(e[k])} == {"with_agent_type"}


@pytest.mark.parametrize("tool", ["cadrl_bench.py", "evaluate.py"])
def test_cadrl_tools_parse_and_show_their_usage(tool, tmp_path):
    import py_compile
    import sys
    path = os.path.join(ROOT, "tools", tool)
    py_compile.compile(path, cfile=str(tmp_path / (tool + "c")), doraise=True)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cadrl" in r.stdout
    if tool == "evaluate.py":
        r = subprocess.run([sys.executable, path, "--policy", "cadrl"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--weights" in r.stderr
