"""SAIL without a GPU: the torch network on the reference's golden run and constructed states, the host build of the
network's arithmetic against them and against torch on the edge batches (also as a program of its own under
AddressSanitizer and UBSan), the facade policy, the refusals and the new ABI entries.  Golden: the reference's own SAIL
(rl/policy/sail.py, torch.manual_seed(11) weights, recorded as arrays) driving the A5 scene, and sixteen constructed states
(tests/golden/sail_a5.npz, sail_cases.npz, tests/golden/make_golden_sail.py)."""
import configparser
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sail_cases import (ADULTS, KINDS, ROOT, TOL_FACTOR, check_kinds, edge_batch, env_counts, golden, golden_weights_file,
                        host_forward, host_group, host_program, layer_arrays, network_inputs, random_state_dict, read_results,
                        ref_error, same_bytes, write_batches)
from ebcsim import _abi, _capi, config as ebc_config

HEADER = os.path.join(ROOT, "include", "ebcsim.h")
PROFILE = os.path.join(ROOT, "profiles", "sail_accuracy.txt")
FILES = ["sail_a5", "sail_cases"]
_accuracy = {}


@pytest.fixture(scope="module", autouse=True)
def accuracy_profile():
    """After the module's tests: profiles/sail_accuracy.txt from what they measured, when both files have been measured."""
    yield
    if len(_accuracy) != len(FILES):
        return
    out = ["# SAIL accuracy, written by tests/test_sail_cpu.py.  e_ref: ExtendedNetwork in torch float32 against a float64 copy of",
           "# the same module, max over every recorded input of the file, for action and for feat_joint; host: the g++ build of",
           "# csrc/ebc_sail_rule.h (what the kernel computes, byte for byte); torch: SailNet on the CPU; both against the",
           "# reference's own recorded outputs; bound = %d * e_ref." % TOL_FACTOR, ""]
    for name in FILES:
        n, e_ref, host, cpu = _accuracy[name]
        for q, what in enumerate(("action", "feat_joint")):
            out.append("%s %s: %d states, e_ref %.3g, |host - recorded| %.3g, |torch - recorded| %.3g (bound %.3g)" % (
                name, what, n, e_ref[q], host[q], cpu[q], TOL_FACTOR * e_ref[q]))
    with open(PROFILE, "w") as f:
        f.write("\n".join(out) + "\n")


def test_policy_factory_serves_sail(tmp_path):
    """configure_env_policy_robot(policy="sail") returns the policy with the reference's attribute surface."""
    from ebcsim.env import configure_env_policy_robot
    from oracle import oracle
    z, meta, sd, _, _ = golden("sail_a5")
    env_path, pol_path = tmp_path / "env.config", tmp_path / "policy.config"
    env_path.write_text(meta["config_text"])
    pol_path.write_text(meta["policy_config_text"])
    env, pol, robot = configure_env_policy_robot(str(env_path), str(pol_path), golden_weights_file(sd, tmp_path), policy="sail",
                                                 backend_factory=lambda p, E, N, S: oracle.OracleEnv(p, E, N, S))
    assert type(pol).__name__ == "SAIL" and pol.name == "SAIL" and pol.trainable and pol.multiagent_training is True
    assert pol.adult_num == 5 and pol.kinematics == "holonomic" and pol.gamma == 0.9 and pol.phase == "test"
    assert list(pol.get_model().state_dict()) == meta["state_dict"]
    assert robot.policy is pol


@pytest.mark.parametrize("name", FILES)
def test_module_loads_the_recorded_state_dict_strictly(name):
    from ebcsim.sail import LAYERS, SailModule
    _, meta, sd, m32, _ = golden(name)
    assert list(sd) == [k + s for k in LAYERS[:-1] for s in (".weight", ".bias")] + ["planner.weight", "planner.bias"]
    assert m32.num_adult == 5 == meta["adult_num"]
    assert SailModule(5).load_state_dict(sd, strict=True).missing_keys == []
    with pytest.raises(RuntimeError):
        SailModule(4).load_state_dict(sd, strict=True)
    w, b = layer_arrays(sd)
    assert [a.shape for a in w] == [(32, 4), (32, 32), (64, 20), (64, 64), (32, 64), (64, 64), (64, 64), (64, 64), (64, 64), (1, 64),
                                    (64, 4), (64, 64), (64, 128), (2, 64)]
    assert sum(a.size for a in w + b) == 38371


@pytest.mark.parametrize("name", FILES)
def test_recorded_outputs_within_the_bound(name):
    """The host build and SailNet on the CPU reproduce every recorded action and feat_joint within TOL_FACTOR * e_ref;
    where the reference returned the arrival action without running the network (`decided` = 0) the action is exactly
    (0, 0) and no feature was recorded."""
    from ebcsim.sail import SailNet
    z, meta, sd, m32, m64 = golden(name)
    robot, ob = z["robot"], z["ob"]
    decided = z["decided"].astype(bool) if "decided" in z.files else np.ones(len(robot), dtype=bool)
    e_ref = ref_error(m32, m64, robot, ob)
    host = host_forward(sd, robot, ob)
    net = SailNet(sd)
    cpu = [t.numpy() for t in net.forward(torch.from_numpy(robot), torch.from_numpy(ob))]
    assert net.device.type == "cpu" and net.native_forwards == 0
    assert cpu[0].dtype == np.float64 and cpu[1].dtype == np.float32 and cpu[0].shape == (len(robot), 2) and cpu[1].shape == (len(robot), 64)
    errs = []
    for got in (host, cpu):
        assert (got[0][~decided] == 0).all() and (z["action"][~decided] == 0).all()
        errs.append((float(np.abs(got[0] - z["action"]).max()), float(np.abs(got[1][decided] - z["feat_joint"][decided]).max())))
    print("%s: e_ref %.3g / %.3g, host %.3g / %.3g, torch %.3g / %.3g (action / feat_joint), bound %d x e_ref" % (
        (name,) + e_ref + errs[0] + errs[1] + (TOL_FACTOR,)))
    _accuracy[name] = (len(robot), e_ref, errs[0], errs[1])
    for err in errs:
        assert err[0] <= TOL_FACTOR * e_ref[0], (err[0], e_ref[0])
        assert err[1] <= TOL_FACTOR * e_ref[1], (err[1], e_ref[1])
    if name == "sail_cases":
        names = meta["names"]
        assert [n for n, d in zip(names, decided) if not d] == ["arrived_inside", "arrived_diagonal_inside"]
        assert np.abs(z["action"][names.index("arrived_outside")]).max() > 0


def _abi_code(info):
    return {"Nothing": _abi.INFO_NOTHING, "Danger": _abi.INFO_DANGER, "ReachGoal": _abi.INFO_REACH_GOAL,
            "CollisionObstacle": _abi.INFO_COLLISION_OBSTACLE, "CollisionAdult": _abi.INFO_COLLISION_ADULT,
            "CollisionBicycle": _abi.INFO_COLLISION_BICYCLE, "CollisionChild": _abi.INFO_COLLISION_CHILD,
            "Timeout": _abi.INFO_TIMEOUT}[type(info).__name__]


def test_policy_reproduces_the_run_step_by_step(tmp_path):
    """rl_policy.SAIL on the oracle env, step by step from the recorded states: at every step the env's own state is the
    recorded one, predict() on the recorded state gives the recorded last_state exactly and the recorded action within the
    bound, and the env stepped with the recorded action gives the recorded reward and info."""
    from ebcsim.action import ActionXY
    from ebcsim.env import configure_env_policy_robot
    from ebcsim.state import FullState, JointState, ObservableState
    from oracle import oracle
    z, meta, sd, m32, m64 = golden("sail_a5")
    env_path, pol_path = tmp_path / "env.config", tmp_path / "policy.config"
    env_path.write_text(meta["config_text"])
    pol_path.write_text(meta["policy_config_text"])
    env, pol, robot = configure_env_policy_robot(str(env_path), str(pol_path), golden_weights_file(sd, tmp_path), policy="sail",
                                                 backend_factory=lambda p, E, N, S: oracle.OracleEnv(p, E, N, S))
    tol = TOL_FACTOR * ref_error(m32, m64, z["robot"], z["ob"])[0]
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    assert len(ob) == meta["rows"] == 5
    T, done = len(z["action"]), False
    for t in range(T):
        assert not done
        np.testing.assert_allclose([[o.px, o.py, o.vx, o.vy, o.radius] for o in ob], z["ob"][t], atol=1e-9, err_msg="step %d" % t)
        np.testing.assert_allclose(robot.get_full_state().px, z["robot"][t][0], atol=1e-9)
        own = robot.act(ob, env=env)  # on the env's own state: the same action up to the casts of a 1e-9 difference
        np.testing.assert_allclose([own[0], own[1]], z["action"][t], atol=1e-5)
        state = JointState(FullState(*[float(x) for x in z["robot"][t]]), [ObservableState(*[float(x) for x in row]) for row in z["ob"][t]])
        action = pol.predict(state, env)
        assert type(action) is ActionXY
        assert np.abs(np.array([action[0], action[1]]) - z["action"][t]).max() <= tol, t
        assert len(pol.last_state) == 2 and pol.last_state[0].dtype == torch.float32 and pol.last_state[1].dtype == torch.float32
        assert np.array_equal(pol.last_state[0].numpy(), z["last_robot"][t]) and np.array_equal(pol.last_state[1].numpy(), z["last_agents"][t]), t
        ob, _, reward, done, info = env.step(ActionXY(*[float(x) for x in z["action"][t]]), compute_local_map=False)
        np.testing.assert_allclose(reward, z["reward"][t], atol=1e-9)
        assert _abi_code(info) == int(z["info"][t]), t
    assert done and _abi_code(info) == int(meta["final_info"])
    assert pol._value_net().native_forwards == 0


def test_policy_checks_and_wrong_agent_count(tmp_path):
    """The reference's three attribute checks in its order, the arrival action before the network, ActionRot for another
    kinematics, and a state with another number of agents raises."""
    from ebcsim.action import ActionRot, ActionXY
    from ebcsim.rl_policy import SAIL
    from ebcsim.state import FullState, JointState, ObservableState
    z, meta, sd, _, _ = golden("sail_cases")
    cfg = configparser.RawConfigParser()
    cfg.read_string(json.loads(str(golden("sail_a5")[0]["meta"]))["policy_config_text"])
    pol = SAIL()
    pol.configure(cfg)
    pol.get_model().load_state_dict(sd)
    names = meta["names"]

    def state_of(i, rows=None):
        return JointState(FullState(*[float(x) for x in z["robot"][i]]),
                          [ObservableState(*[float(x) for x in row]) for row in (z["ob"][i] if rows is None else rows)])
    with pytest.raises(AttributeError, match="Phase"):
        pol.predict(state_of(0))
    pol.set_phase("train")
    with pytest.raises(AttributeError, match="Device"):
        pol.predict(state_of(0))
    pol.set_device("cpu")
    with pytest.raises(AttributeError, match="Epsilon"):
        pol.predict(state_of(0))
    pol.set_phase("test")
    a = pol.predict(state_of(names.index("arrived_inside")))
    assert type(a) is ActionXY and (a[0], a[1]) == (0, 0)
    a = pol.predict(state_of(names.index("arrived_outside")))
    assert type(a) is ActionXY and abs(a[0]) + abs(a[1]) > 0
    for rows in (z["ob"][0][:4], np.concatenate([z["ob"][0], z["ob"][1][:1]])):
        with pytest.raises(ValueError, match="adult_num"):
            pol.predict(state_of(0, rows))
    pol.kinematics = "unicycle"
    assert type(pol.predict(state_of(0))) is ActionRot


def test_refusals_of_adult_num():
    """adult_num 1 and 33 are refused by name: by the entry before a device is touched, and by the Python layers."""
    from ebcsim.sail import SailModule, SailNet, check_adult_num
    lib = _capi.lib()
    w, b = layer_arrays(random_state_dict(2))

    def create(n, size=None):
        s = _abi.EbcSailWeights()
        s.struct_size = C.sizeof(s) if size is None else size
        s.adult_num = n
        for i in range(_abi.SAIL_LAYERS):
            s.weight[i], s.bias[i] = w[i].ctypes.data, b[i].ctypes.data
        h = C.c_void_p()
        return lib.ebc_sail_create(C.addressof(s), 0, C.byref(h))
    assert create(1) == _abi.ERR_UNSUPPORTED and b"adult_num < 2" in lib.ebc_last_error()
    assert create(33) == _abi.ERR_UNSUPPORTED and b"adult_num > 32" in lib.ebc_last_error()
    assert create(0) == _abi.ERR_UNSUPPORTED and create(-4) == _abi.ERR_UNSUPPORTED
    assert create(5, size=8) == _abi.ERR_INVALID and b"struct_size" in lib.ebc_last_error()
    assert lib.ebc_sail_create(None, 0, None) == _abi.ERR_INVALID
    assert lib.ebc_sail_forward(None, None, None) == _abi.ERR_INVALID and lib.ebc_sail_destroy(None) == 0
    for n in (1, 33):
        with pytest.raises(NotImplementedError, match="adult_num"):
            check_adult_num(n)
        with pytest.raises(NotImplementedError):
            SailNet(SailModule(n).state_dict())
    cfg = configparser.RawConfigParser()
    cfg.read_string(json.loads(str(golden("sail_a5")[0]["meta"]))["policy_config_text"])
    cfg.set("sail", "adult_num", "1")
    from ebcsim.rl_policy import SAIL
    with pytest.raises(NotImplementedError):
        SAIL().configure(cfg)


@pytest.mark.parametrize("N", ADULTS)
def test_host_build_against_torch_on_the_edge_batches(N):
    """The g++ build of ebc_sail_rule.h on every edge batch of this adult_num (both weight scales, R = N and N + 3): what
    every kind promises, torch's module within TOL_FACTOR * e_ref on the envs the network decides, padding rows reaching
    nothing, an env's result independent of its place, n_rows = NULL meaning adult_num everywhere.  e_ref is a maximum
    over a set of states (the issue's: every recorded input of a run, tens of states); one env's own difference can be a
    tenth of it, so it is measured once per weight set on the decided envs of a 70-env batch of the same distribution."""
    from ebcsim.sail import SailModule, envs_per_workgroup
    assert host_group(N) == envs_per_workgroup(N)
    seen = set()
    for scale in (1, 8):
        sd = random_state_dict(N, scale)
        m32, m64 = SailModule.from_state_dict(sd).eval(), SailModule.from_state_dict(sd).double().eval()
        robot, ob, _, kinds = edge_batch(N, 70, N, seed=4242 + N)
        sample = np.array([k in ("plain", "equal_logits", "still") for k in kinds])
        e_ref = ref_error(m32, m64, robot[sample], ob[sample])
        for R in (N, N + 3):
            for E in env_counts(N):
                robot, ob, n_rows, kinds = edge_batch(N, E, R)
                seen.update(kinds)
                action, feat = host_forward(sd, robot, ob, n_rows)
                tag = "N %d E %d R %d x%d" % (N, E, R, scale)
                check_kinds(action, feat, n_rows, kinds, N, tag)
                live = np.array([k in ("plain", "equal_logits", "still") for k in kinds])
                if live.any():
                    r, c = network_inputs(robot[live], ob[live], N)
                    with torch.no_grad():
                        a32, f32 = m32(r, c)
                    assert np.abs(a32.numpy() - action[live]).max() <= TOL_FACTOR * e_ref[0], tag
                    assert np.abs(f32.numpy() - feat[live]).max() <= TOL_FACTOR * e_ref[1], tag
                # padding rows reach nothing: other values there, the same bytes
                if R > N:
                    ob2 = ob.copy()
                    ob2[:, N:] = 12345.0
                    a2, f2 = host_forward(sd, robot, ob2, n_rows)
                    assert same_bytes(a2, action) and same_bytes(f2, feat), tag
                # NULL row counts: every env has adult_num rows
                a3, f3 = host_forward(sd, robot, ob, None)
                a4, f4 = host_forward(sd, robot, ob, np.full((E,), N, dtype=np.int64))
                assert same_bytes(a3, a4) and same_bytes(f3, f4), tag
                # an env alone gives the bytes it gives inside the batch
                e = E // 2
                a5, f5 = host_forward(sd, robot[e:e + 1], ob[e:e + 1], n_rows[e:e + 1])
                assert same_bytes(a5[0], action[e]) and same_bytes(f5[0], feat[e]), tag
    assert seen == set(KINDS)


def test_softmax_of_equal_logits_and_a_spread_one():
    """Identical agents give identical rows, equal logits and a uniform softmax: the crowd feature is the one pairwise
    feature, so the host build's action is torch's on that env within the bound; with the attention weights scaled by 8
    the scores of random agents differ, and the two weight sets give different actions."""
    from ebcsim.sail import SailModule
    N = 5
    robot, ob, n_rows, kinds = edge_batch(N, 9, N)
    e = kinds.index("equal_logits")
    out = {}
    for scale in (1, 8):
        sd = random_state_dict(N, scale)
        out[scale] = host_forward(sd, robot, ob)[0]
        m32, m64 = SailModule.from_state_dict(sd).eval(), SailModule.from_state_dict(sd).double().eval()
        r, c = network_inputs(robot[e:e + 1], ob[e:e + 1], N)
        with torch.no_grad():
            a32 = m32(r, c)[0].numpy()
        assert np.abs(a32 - out[scale][e]).max() <= TOL_FACTOR * ref_error(m32, m64, robot[e:e + 1], ob[e:e + 1])[0]
    p = kinds.index("plain")
    assert np.abs(out[1][p] - out[8][p]).max() > 1e-5
    assert np.abs(out[1][e] - out[8][e]).max() < 1e-6  # uniform scores whatever the logits' scale


def test_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/sail_host.cc as a program of its own with -fsanitize=address,undefined on every edge batch: no finding
    (a finding ends the program with a non-zero status), and the bytes of the library build."""
    batches = []
    for N in ADULTS:
        for scale in (1, 8):
            sd = random_state_dict(N, scale)
            for R in (N, N + 3):
                for E in env_counts(N):
                    robot, ob, n_rows, _ = edge_batch(N, E, R)
                    batches.append((sd, robot, ob, n_rows))
    batches += [(b[0], b[1], b[2], None) for b in batches[:4]]
    z, _, sd, _, _ = golden("sail_cases")
    batches.append((sd, z["robot"], z["ob"], None))
    src, dst = str(tmp_path / "edges.bin"), str(tmp_path / "out.bin")
    write_batches(src, batches)
    r = subprocess.run([host_program(sanitize=True), src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d batches" % len(batches) in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    for (sd, robot, ob, nr), (action, feat) in zip(batches, read_results(dst, batches)):
        want = host_forward(sd, robot, ob, nr)
        assert same_bytes(action, want[0]) and same_bytes(feat, want[1]), ob.shape
    raw = open(src, "rb").read()
    open(src, "wb").write(raw[:len(raw) - 5])
    r = subprocess.run([host_program(sanitize=True), src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "malformed" in r.stderr


def test_sail_entries_in_header_and_bindings(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, n_args in (("ebc_sail_create", 3), ("ebc_sail_forward", 3), ("ebc_sail_destroy", 1)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int
    assert "#define EBC_ABI_VERSION 1" in text and _abi.ABI_VERSION == 1
    for struct in ("EbcSailWeights", "EbcSailArgs"):
        S = getattr(_abi, struct)
        fields = [f[0] for f in S._fields_]
        src = tmp_path / (struct + ".c")
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",sizeof(%s));\n%s\nprintf("\\n");return 0;}\n'
                       % (HEADER, struct, "\n".join('printf(" %%zu",offsetof(%s,%s));' % (struct, f) for f in fields)))
        exe = tmp_path / struct
        subprocess.check_call(["gcc", "-o", str(exe), str(src)])
        sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
        assert sizes == [C.sizeof(S)] + [getattr(S, f).offset for f in fields], struct
        assert fields[0] == "struct_size"
    assert _abi.SAIL_LAYERS == 14 and "#define EBC_SAIL_LAYERS 14" in text


def test_params_from_config_takes_sail():
    path = os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config")
    pol = ebc_config.read_config(path)
    assert pol.getboolean("sarl", "with_agent_type")
    _, meta, _, _, _ = golden("sail_a5")
    env_cfg = configparser.RawConfigParser()
    env_cfg.read_string(meta["config_text"])
    default = ebc_config.params_from_config(env_cfg, pol)
    sail = ebc_config.params_from_config(env_cfg, pol, policy="sail")
    assert default.with_agent_type == 1 and sail.with_agent_type == 0
    d, e = ebc_config.params_to_dict(default), ebc_config.params_to_dict(sail)
    assert {k for k in d if json.dumps(d[k]) != json.dumps(e[k])} == {"with_agent_type"}


@pytest.mark.parametrize("tool", ["sail_bench.py", "evaluate.py"])
def test_sail_tools_parse_and_show_their_usage(tool, tmp_path):
    import py_compile
    import sys
    path = os.path.join(ROOT, "tools", tool)
    py_compile.compile(path, cfile=str(tmp_path / (tool + "c")), doraise=True)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "sail" in r.stdout
    if tool == "evaluate.py":
        r = subprocess.run([sys.executable, path, "--policy", "sail"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--weights" in r.stderr
