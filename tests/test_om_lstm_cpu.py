"""OM-LSTM without a GPU: the golden runs of the reference's LstmRL with with_om = true through the facade
(policy="om_lstm_rl") on the oracle backend; ebcsim.occupancy.wide_state_sorted (the state OM-LSTM stores in RL: the rows
sorted by decreasing distance, the maps built from the rows in that order) against "permute, then wide_state", with ties,
NaN keys, padding, and the scene in which the order of a cell's sum shows; what LstmRL and OmLstmRL refuse; LstmTrainer's
autograd path on 61-wide rows; the host builds of the LSTM rules at row widths 61 and 64.  Cases and bars:
tests/om_lstm_cases.py."""
import configparser
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lstm_grad_cases as lg
import om_lstm_cases as oc
from lstm_cases import F_CELL, host_lstm, lstm_case, lstm_weights, torch_h_n
from om_cases import compare_maps
from ebcsim import _abi, _capi
from ebcsim.occupancy import OccupancySpec, distance_order, occupancy_maps, wide_state, wide_state_sorted

ROOT = oc.ROOT
HEADER = os.path.join(ROOT, "include", "ebcsim.h")


def same(a, b, tag=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8), err_msg=str(tag))


# ---------------------------------------------------------------------- 1. the golden runs
def _facade(meta, tmp_path, policy="om_lstm_rl"):
    from ebcsim.env import configure_env_policy_robot
    from oracle import oracle
    env_path, pol_path = tmp_path / "env.config", tmp_path / "policy.config"
    env_path.write_text(meta["config_text"])
    pol_path.write_text(meta["policy_config_text"])
    return configure_env_policy_robot(str(env_path), str(pol_path), oc.golden_weights_file(meta, tmp_path), phase="train",
                                      policy=policy, backend_factory=lambda p, E, N, S: oracle.OracleEnv(p, E, N, S))


def _abi_code(info):
    return {"Nothing": _abi.INFO_NOTHING, "Danger": _abi.INFO_DANGER, "ReachGoal": _abi.INFO_REACH_GOAL,
            "CollisionObstacle": _abi.INFO_COLLISION_OBSTACLE, "CollisionAdult": _abi.INFO_COLLISION_ADULT,
            "CollisionBicycle": _abi.INFO_COLLISION_BICYCLE, "CollisionChild": _abi.INFO_COLLISION_CHILD,
            "Timeout": _abi.INFO_TIMEOUT}[type(info).__name__]


@pytest.mark.parametrize("name", oc.RUNS)
def test_om_lstm_facade_run(name, tmp_path):
    """configure_env_policy_robot(..., policy="om_lstm_rl") on the oracle backend, phase "train", epsilon 0: the recorded
    action at EVERY decision, the 81 values within F_CELL x e_ref (LstmModule float32 against its float64 copy on the rows
    the policy built, measured here), last_state [R, 61] = the recorded one (13 columns at the rotate tolerance, the maps by
    compare_maps), reward and info; one sweep per decision."""
    z, meta, spec, m32, m64 = oc.golden_run(name)
    env, pol, robot = _facade(meta, tmp_path)
    assert type(pol).__name__ == "OmLstmRL" and pol.name == "OM-LSTM-RL" and pol.with_om is True
    assert pol.input_dim() == 13 + spec.width == meta["input_dim"] == 61 and pol.spec() == spec
    assert list(pol.get_model().state_dict()) == [k for k, _, _ in meta["state_dict"]]
    pol.set_epsilon(0.0)
    ob, _ = env.reset("test", test_case=meta["seed_case"], compute_local_map=False)
    assert len(ob) == meta["rows"]
    net, seen = pol._value_net(), []
    forward = net.action_values
    net.action_values = lambda rows, *a, **kw: (seen.append(oc.value_error(m32, m64, rows)), forward(rows, *a, **kw))[1]
    done, t, err = False, 0, 0.0
    while not done:
        assert t < len(z["action"])
        calls = env.backend_calls
        action = robot.act(ob, env=env)
        assert env.backend_calls == calls + 1 and len(seen) == t + 1  # one sweep per decision
        np.testing.assert_allclose([action[0], action[1]], z["action"][t], atol=1e-12, err_msg="decision %d" % t)
        err = max(err, float(np.abs(np.array(pol.action_values) - z["values"][t]).max()))
        last = pol.last_state.numpy()
        assert last.shape == (meta["rows"], 61) and last.dtype == np.float32
        np.testing.assert_allclose(last[:, :13], z["last_state"][t][:, :13], atol=oc.ROTATE_TOL, rtol=oc.ROTATE_TOL, err_msg="decision %d" % t)
        compare_maps(last[:, 13:], z["last_state"][t][:, 13:], spec)
        ob, _, reward, done, info = env.step(action, compute_local_map=False)
        np.testing.assert_allclose(reward, z["reward"][t], atol=1e-9)
        assert _abi_code(info) == int(z["info"][t]), t
        t += 1
    assert t == len(z["action"]) and _abi_code(info) == int(meta["final_info"])
    top = np.sort(z["values"], axis=1)
    gap = float((top[:, -1] - top[:, -2]).min())
    print("%s: %d decisions, e_ref %.3g, |values - recorded| %.3g (bound %.3g), gap %.3g" % (name, t, max(seen), err, F_CELL * max(seen), gap))
    assert err <= F_CELL * max(seen), (err, max(seen))


@pytest.mark.parametrize("name", oc.RUNS)
def test_goldens_hold_what_their_generator_promises(name):
    """No decision is left out: every recorded state keeps MARGIN cells off the cell boundaries and every top-2 gap is above
    twice the recorded tolerance; the recorded maps of predict() are the product's on the recorded rows, and last_state's
    are the product's on the recorded SORTED rows — not a permutation of the env-order maps where the orders differ."""
    from om_cases import MARGIN
    from ebcsim.occupancy import boundary_margin
    z, meta, spec, _, _ = oc.golden_run(name)
    assert meta["closest_boundary"] >= MARGIN and meta["top2_gap"] > 2 * 8 * meta["float32_error"]
    for key in ("om_ob", "last_ob"):
        assert float(boundary_margin(z[key], None, spec).min()) >= MARGIN
    compare_maps(occupancy_maps(z["om_ob"], None, spec), z["om"], spec)
    compare_maps(occupancy_maps(z["last_ob"], None, spec), np.ascontiguousarray(z["last_state"][:, :, 13:]), spec)
    assert (np.diff(z["last_state"][:, :, 11], axis=1) < 0).all()  # recorded in strictly decreasing float32 distance
    # wide_state_sorted on the recorded rows, shuffled: the recorded state again (the 13 columns byte for byte: they are copied)
    rs = np.random.RandomState(3)
    N, R = z["last_ob"].shape[:2]
    perm = np.stack([rs.permutation(R) for _ in range(N)])[:, :, None]
    rot = np.take_along_axis(np.ascontiguousarray(z["last_state"][:, :, :13]), perm, axis=1)
    ob = np.take_along_axis(z["last_ob"], perm, axis=1)
    got = wide_state_sorted(rot, ob, None, spec)
    same(got[:, :, :13], np.ascontiguousarray(z["last_state"][:, :, :13]), "the rotated columns")
    compare_maps(np.ascontiguousarray(got[:, :, 13:]), np.ascontiguousarray(z["last_state"][:, :, 13:]), spec)


# ---------------------------------------------------------------------- 2. wide_state_sorted
def _random_states(seed, E=12, R=7, T=13):
    rs = np.random.RandomState(seed)
    ob = np.zeros((E, R, 5))
    ob[:, :, :2] = rs.uniform(-2.0, 2.0, (E, R, 2))
    ob[:, :, 2:4] = rs.normal(0.0, 0.8, (E, R, 2))
    ob[:, :, 4] = 0.3
    rot = rs.normal(0.0, 1.0, (E, R, T)).astype(np.float32)
    rot[:, :, 11] = np.hypot(ob[:, :, 0], ob[:, :, 1]).astype(np.float32)
    nv = rs.randint(0, R + 1, E).astype(np.int64)
    nv[:4] = [0, 1, R, R + 3]
    return rot, ob, nv


@pytest.mark.parametrize("spec", [OccupancySpec(4, 1.0, 3), OccupancySpec(1, 3.0, 1), OccupancySpec(3, 0.5, 2)], ids=str)
def test_wide_state_sorted_is_permute_then_wide_state(spec):
    """Random ragged states with ties and NaN keys: wide_state_sorted is wide_state of the rows permuted by the stable
    descending order of their float32 distance column; its first T columns are sort_rows_by_distance's bytes; NaN keys go
    behind every number in the env's order; padding slots stay put with zero maps."""
    from ebcsim.lstm_train import sort_rows_by_distance
    rot, ob, nv = _random_states(31 + spec.width)
    E, R, T = rot.shape
    rot[4, 1, 11] = rot[4, 3, 11]                      # a tie keeps the env's order
    rot[5, 0, 11] = rot[5, 2, 11] = np.nan             # NaN keys go last, in the env's order
    nv[4], nv[5] = R, R
    for e in range(E):                                 # padding that would win every comparison
        rot[e, max(0, min(R, nv[e])):, 11] = (1e30, np.inf, np.nan)[e % 3]
    got = wide_state_sorted(rot, ob, nv, spec)
    assert got.dtype == np.float32 and got.shape == (E, R, T + spec.width)
    same(got[:, :, :T], sort_rows_by_distance(torch.from_numpy(rot), torch.from_numpy(nv)).numpy(), "the first T columns")
    order = distance_order(rot, nv)
    for e in range(E):
        n = int(np.clip(nv[e], 0, R))
        assert order[e, n:].tolist() == list(range(n, R)) and sorted(order[e, :n].tolist()) == list(range(n))
        key = rot[e, order[e, :n], 11]
        num = key[~np.isnan(key)]
        assert (np.diff(num) <= 0).all() and not np.isnan(key[:len(num)]).any()
        want = wide_state(rot[e:e + 1, order[e]], ob[e:e + 1, order[e]], nv[e:e + 1], spec)[0]
        same(got[e], want, e)
        same(got[e, n:, :T], rot[e, n:], "padding rows stay")
        assert not got[e, n:, T:].any()
    assert order[4].tolist().index(1) + 1 == order[4].tolist().index(3)
    assert order[5, -2:].tolist() == [0, 2]
    same(wide_state_sorted(rot[:, :, :], ob, None, spec)[2], got[2], "n_valid None = all R")


def test_the_order_of_a_cells_sum_is_the_sorted_one():
    """Three occupants of one cell of row 3's map with vx = 2^60, 1, -2^60; by distance they sort 0, 2, 1: the cell's mean
    is (2^60 - 2^60 + 1) / 3 in the sorted order; the permuted wide_state has the env order's (2^60 + 1 - 2^60) / 3 = 0."""
    rot, ob = oc.rotated_of(oc.ORDER_SCENE), oc.ob_of(oc.ORDER_SCENE)
    assert distance_order(rot[None])[0].tolist() == oc.ORDER_SORTED != list(range(4))
    got = wide_state_sorted(rot[None], ob[None], None, oc.OM)[0]
    permuted = wide_state(rot[None], ob[None], None, oc.OM)[0][oc.ORDER_SORTED]
    same(got[:, :13], permuted[:, :13], "the rotated columns are a permutation")
    assert oc.order_cell_means(got[3]) == (1.0, float(np.float32(1.0 / 3.0)), 0.0)
    assert oc.order_cell_means(permuted[3]) == (1.0, 0.0, 0.0)
    assert not np.array_equal(got, permuted)
    # and on the reference's own arithmetic: the float64 sum in list order, divided by the count, cast once
    assert np.float32(((oc.BIG + -oc.BIG) + 1.0) / 3.0) == got[3, 13 + 3 * oc.ORDER_CELL + 1]


def test_mirrored_rows_keep_the_envs_order():
    rot, ob = oc.rotated_of(oc.MIRROR_SCENE), oc.ob_of(oc.MIRROR_SCENE)
    assert rot[0, 11] == rot[1, 11] and rot[2, 11] > rot[0, 11]
    assert distance_order(rot[None])[0].tolist() == oc.MIRROR_SORTED
    got = wide_state_sorted(rot[None], ob[None], None, oc.OM)[0]
    same(got[:, :13], rot[oc.MIRROR_SORTED])


# ---------------------------------------------------------------------- 3. the policy objects
def _policy_cfg(meta, **lstm):
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["policy_config_text"])
    for k, v in lstm.items():
        sec, key = k.split("__") if "__" in k else ("lstm_rl", k)
        cfg.set(sec, key, v)
    return cfg


def test_lstm_rl_keeps_refusing_and_om_lstm_rl_refuses_the_rest():
    from ebcsim.env import _policy_factory
    from ebcsim.rl_policy import LstmRL, OmLstmRL
    from ebcsim import config as ebc_config
    _, meta, spec, _, _ = oc.golden_run(oc.RUNS[0])
    assert _policy_factory()["om_lstm_rl"] is OmLstmRL and _policy_factory()["lstm_rl"] is LstmRL
    with pytest.raises(NotImplementedError, match="OmLstmRL"):
        LstmRL().configure(_policy_cfg(meta))
    with pytest.raises(ValueError, match="LstmRL"):
        OmLstmRL().configure(_policy_cfg(meta, with_om="false"))
    with pytest.raises(NotImplementedError, match="64"):
        OmLstmRL().configure(_policy_cfg(meta, om__cell_num="5"))  # 13 + 75
    with pytest.raises(NotImplementedError, match="query_env"):
        OmLstmRL().configure(_policy_cfg(meta, action_space__query_env="false"))
    pol = OmLstmRL()
    pol.configure(_policy_cfg(meta))
    assert pol.name == "OM-LSTM-RL" and pol.input_dim() == 61 and pol.spec() == spec == oc.OM and pol.with_agent_type is False
    assert pol.get_model().input_dim == 61 and pol.get_model().with_interaction_module
    plain = OmLstmRL()
    plain.configure(_policy_cfg(meta, with_interaction_module="false"))
    assert tuple(plain.get_model().lstm.weight_ih_l0.shape) == (200, 61)  # ValueNetwork1: the cell's input is 61 wide
    # the tables that never read with_agent_type, and the spec a policy config asks for
    env_cfg = configparser.RawConfigParser()
    env_cfg.read_string(meta["config_text"])
    typed = ebc_config.read_config(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_agent_type.config"))
    assert ebc_config.params_from_config(env_cfg, typed).with_agent_type == 1
    assert bytes(ebc_config.params_from_config(env_cfg, typed, policy="om_lstm_rl")) == bytes(ebc_config.params_from_config(env_cfg, typed, policy="lstm_rl"))
    assert ebc_config.occupancy_from_config(_policy_cfg(meta), policy="om_lstm_rl") == spec
    assert ebc_config.occupancy_from_config(_policy_cfg(meta, with_om="false"), policy="om_lstm_rl") is None
    assert ebc_config.occupancy_from_config(_policy_cfg(meta), policy="lstm_rl") is None
    shipped = ebc_config.read_config(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_om_lstm.config"))
    assert ebc_config.occupancy_from_config(shipped, policy="om_lstm_rl") == oc.OM
    OmLstmRL().configure(shipped)


def test_value_net_takes_61_wide_rows_and_names_the_limit():
    """LstmValueNet on the CPU is LstmModule at width 61, with mlp1 and without; a row of another width is a ValueError, and a
    network wider than 64 is refused by name wherever it would have to run in the library."""
    from ebcsim.lstm_rl import LstmValueNet
    from ebcsim.lstm_rl import LstmModule
    for ni in (2, 3):
        net = oc.GRAD_NETS[ni]
        sd = lg.random_state_dict(net)
        vn = LstmValueNet(sd)
        vn.check_native_width()
        rows, _ = lg.plain_batch(net, 5, 4)
        with torch.no_grad():
            want = LstmModule.from_state_dict(sd)(torch.from_numpy(rows)).squeeze(1)
        assert vn.input_dim == 61 and torch.equal(vn.forward(torch.from_numpy(rows)), want)
        with pytest.raises(ValueError, match="61"):
            vn.forward(torch.zeros((2, 3, 13)))
    too_wide = lg.random_state_dict(oc.wide(lg.NARROW_NET1, 65))
    with pytest.raises(NotImplementedError, match="64"):
        LstmValueNet(too_wide).check_native_width()


# ---------------------------------------------------------------------- 4. trainer and schedule
@pytest.mark.parametrize("ni", [0, 1], ids=["mlp1", "plain"])
def test_autograd_trainer_on_61_wide_rows_steps_as_torch_does(ni):
    """LstmTrainer(native=False) on a 61-wide network: three SGD steps (momentum 0.9) on an edge batch move the weights
    exactly as torch.optim.SGD moves LstmModule's parameters on the same loss."""
    from ebcsim.lstm_train import LstmTrainer, module_of
    net = oc.GRAD_NETS[ni]
    assert net[0][0] == 61
    sd = lg.random_state_dict(net)
    rows, target, nv, mask, _ = lg.edge_batch(net, 9, 5)
    target = np.nan_to_num(target)
    live = lg.is_live(nv, mask)
    tr = LstmTrainer(sd, device="cpu", optimizer="sgd", lr=0.05, native=False)
    assert tr.widths[0] == 61 and tr.with_interaction_module == net[2]
    m = module_of(sd)
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
    idx = np.nonzero(live)[0]
    x = torch.from_numpy(rows[idx].copy())
    n = torch.from_numpy(np.clip(nv[idx], 0, 5))
    x[torch.arange(5)[None, :] >= n[:, None]] = 0.0
    y = torch.from_numpy(target[idx])
    for step in range(3):
        loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
        tr.step()
        opt.zero_grad()
        d = m(x, n).squeeze(1) - y
        (0.5 * (2.0 / len(idx)) * (d * d).sum()).backward()
        opt.step()
        assert int(count) == len(idx) and abs(float(loss) - float((d.detach().double() ** 2).sum())) <= 1e-12
        now = tr.state_dict()
        for k, v in m.state_dict().items():
            assert torch.equal(now[k], v), (step, k)
    assert not all(torch.equal(now[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="61"):
        tr.loss_and_grad(torch.zeros(1, 2, 13), torch.zeros(1))


def test_collect_refuses_sorted_rows_without_maps_by_name():
    from ebcsim.train import collect
    with pytest.raises(ValueError, match="sorted_rows needs om"):
        collect(None, None, None, None, 1, 0.9, sorted_rows=True)
    with pytest.raises(ValueError, match="state_transform"):
        collect(None, None, None, None, 1, 0.9, om=oc.OM, sorted_rows=True, state_transform=lambda r, n: r)


# ---------------------------------------------------------------------- 5. the host builds at 61 and 64 columns
@pytest.mark.parametrize("T", oc.WIDTHS + [65])
def test_grad_host_build_at_the_wide_row_widths(T, tmp_path):
    """tests/native/lstm_grad_host.cc at row width 61 and 64, both narrow networks: the library build and the program give
    the same bytes on plain and edge batches, and the rule holds the accuracy bar; width 65 is refused with code 1 by the
    header, and the program ends with exit status 1 on such a batch."""
    L = lg.host_lib()
    nets = [oc.wide(lg.NARROW_NET2, T), oc.wide(lg.NARROW_NET1, T)]
    if T == 65:
        for net in nets:
            assert int(L.lstm_grad_host_refused(lg._w(net[0]).ctypes.data, net[1], int(net[2]))) == 1
        src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        rows, target = lg.plain_batch(nets[0], 1, 1)
        lg.write_batches(src, [(nets[0], np.zeros(16, np.float32), rows, target, None, None, 1.0)])
        run = subprocess.run([lg.host_program(), src, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert run.returncode == 1, run.stdout.decode()
        return
    batch_list, want = [], []
    for net in nets:
        assert int(L.lstm_grad_host_refused(lg._w(net[0]).ctypes.data, net[1], int(net[2]))) == 0
        P = lg.host_pack(lg.random_state_dict(net))
        for B, R in ((9, 5), (3, 1), (5, 2)):
            rows, target, nv, mask, _ = lg.edge_batch(net, B, R)
            batch_list.append((net, P, rows, target, nv, mask, 2.0 / B))
            rows, target = lg.plain_batch(net, B, R)
            batch_list.append((net, P, rows, target, None, None, 2.0 / B))
        want += [lg.host_grad(b[1], b[0], b[2], b[3], b[4], b[5], b[6]) for b in batch_list[len(want):]]
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    lg.write_batches(src, batch_list)
    run = subprocess.run([lg.host_program(), src, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert run.returncode == 0, run.stdout.decode()
    for got, w in zip(lg.read_results(out, batch_list), want):
        assert lg.same_bytes(got[0], w[0]) and np.float64(got[1]).tobytes() == np.float64(w[1]).tobytes() and got[2] == w[2]
        assert lg.same_bytes(got[3], w[3]) and lg.same_bytes(got[4], w[4])


@pytest.mark.parametrize("case", oc.accuracy_cases(), ids=oc.case_name)
def test_the_rule_on_wide_rows_against_float64_autograd(case):
    """Per parameter tensor and for the loss: the host build's error against float64 autograd is within 8 x torch's own
    float32 error, floored at 2^-25."""
    tensors, loss = oc.accuracy_row(case)
    for key, er, et, bar in tensors + [("loss_sum",) + loss]:
        print("%-34s %-22s rule %.3e torch32 %.3e bar %.3e" % (oc.case_name(case), key, er, et, bar))
    for key, er, et, bar in tensors + [("loss_sum",) + loss]:
        assert er <= bar, (key, er, et, bar)


@pytest.mark.parametrize("I", oc.WIDTHS)
def test_cell_host_build_at_the_wide_row_widths(I):
    """tests/native/lstm_host.cc with a cell input 61 and 64 wide (ValueNetwork1 on wide rows), H = 50: h_n against
    torch.nn.LSTM in float64 within F_CELL x torch's own float32 error; NaN-filled padding never reaches it."""
    for R, scale in ((1, 1.0), (5, 1.0), (18, 4.0)):
        lstm, x_nan, x_zero, nv = lstm_case(I, 50, R, scale)
        B = x_nan.shape[0]
        ref = torch_h_n(lstm, x_zero, nv, torch.float64)
        f32 = torch_h_n(lstm, x_zero, nv, torch.float32)
        got = host_lstm(lstm_weights(lstm), x_nan.numpy(), nv.numpy(), B, R)
        assert np.isfinite(got).all() and (got[nv.numpy() == 0] == 0).all()
        e_ref, e_cell = float(np.abs(f32 - ref).max()), float(np.abs(got - ref).max())
        print("I %d R %d scale %g: e_ref %.3g e_cell %.3g" % (I, R, scale, e_ref, e_cell))
        assert e_cell <= F_CELL * e_ref


# ---------------------------------------------------------------------- 6. the entry, the tools, the config
def test_entry_in_header_and_bindings():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+ebc_observe_wide_sorted\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 4 == len(_capi.SYMBOLS["ebc_observe_wide_sorted"][1])
    assert _capi.SYMBOLS["ebc_observe_wide_sorted"] == _capi.SYMBOLS["ebc_observe_wide"]
    assert hasattr(_capi.lib(), "ebc_observe_wide_sorted")
    lib = _capi.lib()
    good = _abi.om_spec(oc.OM)
    assert lib.ebc_observe_wide_sorted(None, C.addressof(good), None, None) != _abi.OK
    short = _abi.om_spec(oc.OM)
    short.struct_size -= 4
    assert lib.ebc_observe_wide_sorted(None, C.addressof(short), None, None) == _abi.ERR_INVALID and b"EbcOmSpec.struct_size" in lib.ebc_last_error()
    assert lib.ebc_observe_wide_sorted(None, None, None, None) == _abi.ERR_INVALID


@pytest.mark.parametrize("tool", ["om_lstm_bench.py", "train_lstm.py", "evaluate.py"])
def test_tools_parse_and_show_their_usage(tool, tmp_path):
    import py_compile
    import sys
    path = os.path.join(ROOT, "tools", tool)
    py_compile.compile(path, cfile=str(tmp_path / (tool + "c")), doraise=True)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    if tool == "evaluate.py":
        pol = os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_om_lstm.config")
        r = subprocess.run([sys.executable, path, "--policy", "lstm_rl", "--policy-config", pol], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--weights" in r.stderr
