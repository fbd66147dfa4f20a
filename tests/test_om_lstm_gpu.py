"""OM-LSTM on the device: ebc_observe_wide_sorted against the composition it replaces and against the numpy form, byte for
byte; constructed scenes (a tie, the scene in which the order of a cell's sum shows); the LDS limit, the refusals and a
capturing stream; ebc_lstm_grad on 61- and 64-wide rows against the host build, byte for byte, and against float64
autograd; DeviceSarlPolicy(LstmValueNet, om=spec) on every golden decision; collect with sorted_rows against the
composition, and without the new arguments against the parent's loop; the schedule end to end.  Cases and bars:
tests/om_lstm_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lstm_grad_cases as lg
import om_lstm_cases as oc
from helpers import batch_from_init, params_of
from lstm_cases import F_CELL
from sail_rollout_cases import params_for
from ebcsim import _abi, _capi, scene as ebc_scene
from ebcsim.occupancy import OccupancySpec, observe_wide_composed, observe_wide_sorted_composed, wide_state_sorted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = oc.ROOT
AUTO = _abi.FLAG_AUTO_RESET
GAMMA = 0.9
OM = oc.OM
SPECS = [OccupancySpec(n, {1: 3.0, 4: 1.0}[n], c) for c in (1, 2, 3) for n in (1, 4)]
# (humans, static rows) per scene: 1, 2, 3, 4 and 2 observation rows
RAGGED = [(1, 0), (1, 1), (2, 1), (3, 1), (2, 0), (3, 0), (1, 1), (3, 1)]


def scenes(seed, E, counts, N=3, S=1, goal=(0.1, 1.5)):
    """E scenes of N human and S static slots of which scene e uses counts[e % len(counts)]; the robot's goal lies
    goal[0] .. goal[1] ahead of it (scene 0: goal[0]); unused slots are zeros.  The shape of tests/test_om_train_gpu.py's."""
    rs = np.random.RandomState(seed)
    f = lambda *s: np.zeros(s)  # noqa: E731
    nh = np.array([counts[e % len(counts)][0] for e in range(E)], np.int32)
    ns = np.array([counts[e % len(counts)][1] for e in range(E)], np.int32)
    b = ebc_scene.SceneBatch(E, N, S, nh, f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                             np.zeros((E, N), np.uint8), ns, f(E, max(S, 1)), f(E, max(S, 1)), f(E, max(S, 1)), None, f(E, 9))
    for e in range(E):
        n, s = int(nh[e]), int(ns[e])
        b.px[e, :n], b.py[e, :n] = rs.uniform(-2.5, 2.5, n), rs.uniform(-2.5, 2.5, n)
        b.vx[e, :n], b.vy[e, :n] = rs.uniform(-0.5, 0.5, n), rs.uniform(-0.5, 0.5, n)
        b.gx[e, :n], b.gy[e, :n] = rs.uniform(-4, 4, n), rs.uniform(-4, 4, n)
        b.radius[e, :n], b.v_pref[e, :n] = rs.uniform(0.1, 0.5, n), rs.uniform(0.3, 1.2, n)
        b.type[e, :n] = np.sort(rs.randint(0, 3, n))
        b.spx[e, :s], b.spy[e, :s], b.sradius[e, :s] = rs.uniform(-2.5, 2.5, s), rs.uniform(-2.5, 2.5, s), rs.uniform(0.3, 0.8, s)
        x, d = rs.uniform(-1, 1), goal[0] if e == 0 else rs.uniform(*goal)
        b.robot[e] = [x, -3.0, 0, 0, 0.3, x, -3.0 + d, 0.7, np.pi / 2]
    return b


def make_env(params, batch, pool=None):
    from ebcsim.batched import BatchedEnv
    env = BatchedEnv(params, batch.n, batch.N, batch.S)
    env.reset(batch)
    if pool is not None:
        env.set_scene_pool(pool)
    env.use_torch_stream()
    return env


def ragged_env(T, kin, E=5, seed=6100):
    return make_env(params_for(T, kin), scenes(seed, E, RAGGED), scenes(seed + 1, 2 * E, RAGGED[3:] + RAGGED[:3]))


def same(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8), err_msg=str(tag))


def observe_sorted(env, spec, with_rows=True, fill=-7.0, offset=0):
    """observe_wide_sorted_device into a poisoned tensor that starts `offset` floats after a 16-byte boundary."""
    total = env.E * env.R * (env.T + spec.width)
    buf = torch.full((total + 8,), fill, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + total].view(env.E, env.R, env.T + spec.width)
    n = torch.full((env.E,), -7, dtype=torch.int64, device=DEV) if with_rows else None
    env.observe_wide_sorted_device(out, spec, n)
    env.synchronize()
    guard = buf.cpu().numpy()
    assert (guard[:offset] == fill).all() and (guard[offset + total:] == fill).all()
    return out.cpu().numpy(), None if n is None else n.cpu().numpy()


def composed(env, spec):
    n = torch.full((env.E,), -7, dtype=torch.int64, device=DEV)
    wide = observe_wide_sorted_composed(env, spec, n_rows=n)
    env.synchronize()
    return wide.cpu().numpy(), n.cpu().numpy()


# ---------------------------------------------------------------------- 1. ebc_observe_wide_sorted
@pytest.mark.parametrize("kin", [_abi.HOLONOMIC, _abi.UNICYCLE], ids=["holonomic", "unicycle"])
@pytest.mark.parametrize("T", [13, 17])
def test_observe_wide_sorted_is_the_composition_in_bytes(T, kin):
    """5 envs of 3 human + 1 static slots, row counts 1 .. 4, a ragged pool; channels 1, 2, 3 x cell_num 1 and 4, at the
    reset state and after two steps with restarts: state_wide and n_rows are the bytes of observe_wide_sorted_composed
    (observe, sort, gather, ebc_occupancy_rows, cat) and of the numpy form wide_state_sorted on ebc_observe's outputs; the
    same bytes into an output that starts one float after a 16-byte boundary (the unaligned head) and without n_rows."""
    env = ragged_env(T, kin)
    act = np.tile([0.4, 0.2], (env.E, 1))
    moved = 0
    for visit in range(3):
        counts = env.row_counts()
        if visit == 0:
            assert sorted(counts.tolist()) == [1, 2, 2, 3, 4] and env.ragged
        ob, rot = env.observe()
        for spec in SPECS:
            got, n = observe_sorted(env, spec)
            want, wn = composed(env, spec)
            same(got, want, (visit, spec))
            same(n, wn, (visit, spec, "n_rows"))
            same(n, counts, (visit, spec, "row_counts"))
            same(got, wide_state_sorted(rot, ob, counts, spec), (visit, spec, "numpy"))
            assert not got[np.arange(env.R)[None, :] >= counts[:, None]].any()  # padding: zero rows, zero maps
            same(observe_sorted(env, spec, with_rows=False, offset=1)[0], want, (visit, spec, "one float off, no n_rows"))
            same(observe_sorted(env, spec, offset=3)[0], want, (visit, spec, "three floats off"))
        key = np.where(np.arange(env.R)[None, :] < counts[:, None], rot[:, :, 11], np.float32(-1.0))  # a distance is >= 0
        moved += int((np.diff(key, axis=1) > 0).any())
        if visit == 0:
            assert any(observe_sorted(env, s)[0][:, :, T:].any() for s in SPECS)  # some map is not empty
        done = env.step(robot_action=act, human_policy=_abi.HUMAN_ORCA, flags=AUTO)["done"]
        assert visit > 0 or done[0]  # env 0 ends at its first step and restarts from the pool
    assert moved > 0  # the env's order was not the sorted one somewhere
    env.close()


def test_constructed_scenes_a_tie_and_the_order_of_a_sum():
    """No step taken.  Env 0: two humans at mirrored positions have the same float32 distance and keep the env's order behind
    the farther third.  Env 1: three occupants of one cell of row 3's map with vx = 2^60, 1, -2^60 sort 0, 2, 1 by distance:
    the cell's mean vx is the sorted order's 1 / 3, not the env order's 0 that a permuted ebc_observe_wide carries."""
    env = make_env(params_for(13), oc.scene_batch([oc.MIRROR_SCENE, oc.ORDER_SCENE]))
    ob, rot = env.observe()
    got, n = observe_sorted(env, OM)
    want, _ = composed(env, OM)
    same(got, want, "composition")
    same(got, wide_state_sorted(rot, ob, n, OM), "numpy")
    assert n.tolist() == [3, 4]
    assert rot[0, 0, 11] == rot[0, 1, 11] < rot[0, 2, 11]
    same(got[0, :3, :13], rot[0, oc.MIRROR_SORTED], "the tie keeps the env's order")
    assert not got[0, 3].any()
    same(got[1, :, :13], rot[1, oc.ORDER_SORTED], "sorted rows")
    assert oc.order_cell_means(got[1, 3]) == (1.0, float(np.float32(1.0 / 3.0)), 0.0)
    plain = torch.empty((2, 4, 13 + OM.width), dtype=torch.float32, device=DEV)
    env.observe_wide_device(plain, OM)
    env.synchronize()
    plain = plain.cpu().numpy()
    same(plain, observe_wide_composed(env, OM).cpu().numpy(), "ebc_observe_wide itself")
    assert oc.order_cell_means(plain[1, 3]) == (1.0, 0.0, 0.0)  # the env's order: (2^60 + 1) - 2^60
    assert not np.array_equal(plain[1, oc.ORDER_SORTED], got[1])
    env.close()


def test_observe_wide_sorted_at_the_lds_limit():
    """R = 128 (33 human + 95 static slots), W = 192 (cell_num 8, 3 channels), T = 17, E = 2, the second env ragged."""
    b = scenes(6200, 2, [(33, 95), (20, 50)], N=33, S=95)
    env = make_env(params_for(17), b)
    spec = OccupancySpec(8, 1.0, 3)
    assert env.R == 128 and spec.width == 192
    got, n = observe_sorted(env, spec, offset=1)
    want, wn = composed(env, spec)
    same(got, want, "limit")
    same(n, wn, "limit n_rows")
    ob, rot = env.observe()
    same(got, wide_state_sorted(rot, ob, n, spec), "limit numpy")
    assert n.tolist() == [128, 70] and got[:, :, 17:].any() and not got[1, 70:].any()
    assert (np.diff(got[0, :, 11]) <= 0).all() and (np.diff(got[1, :70, 11]) <= 0).all() and (np.diff(rot[0, :, 11]) > 0).any()
    env.close()


def test_observe_wide_sorted_refusals_and_capture():
    """channels outside {1, 2, 3}, cell_num 0, a cell_size that is not a finite positive number, W > 192, NULL output,
    a bad struct_size, before ebc_reset, a capturing stream: refused under the entry's own name with nothing written;
    usable afterwards.  The capture is begun and ended, never replayed."""
    from ebcsim.batched import BatchedEnv
    lib = _capi.lib()
    raw = BatchedEnv(params_for(17), 2, 3, 1)
    buf = torch.full((4096,), -5.0, dtype=torch.float32, device=DEV)
    good = _abi.om_spec(OM)
    assert lib.ebc_observe_wide_sorted(raw._h, C.addressof(good), buf.data_ptr(), None) == _abi.ERR_STATE
    assert b"ebc_observe_wide_sorted before ebc_reset" in lib.ebc_last_error()
    raw.close()
    env = ragged_env(17, _abi.HOLONOMIC)
    for change, word in ((dict(channels=0), b"channels"), (dict(channels=4), b"channels"), (dict(cell_num=0), b"cell_num < 1"),
                         (dict(cell_num=9), b"W > 192"), (dict(cell_size=0.0), b"cell_size"), (dict(cell_size=-1.0), b"cell_size"),
                         (dict(cell_size=float("inf")), b"cell_size"), (dict(cell_size=float("nan")), b"cell_size")):
        s = _abi.om_spec(OM)
        for k, v in change.items():
            setattr(s, k, v)
        assert lib.ebc_observe_wide_sorted(env._h, C.addressof(s), buf.data_ptr(), None) == _abi.ERR_UNSUPPORTED, change
        assert word in lib.ebc_last_error() and b"ebc_observe_wide_sorted: " in lib.ebc_last_error(), (change, lib.ebc_last_error())
    assert lib.ebc_observe_wide_sorted(env._h, C.addressof(good), None, None) == _abi.ERR_INVALID and b"state_wide is NULL" in lib.ebc_last_error()
    short = _abi.om_spec(OM)
    short.struct_size -= 4
    assert lib.ebc_observe_wide_sorted(env._h, C.addressof(short), buf.data_ptr(), None) == _abi.ERR_INVALID
    assert b"EbcOmSpec.struct_size" in lib.ebc_last_error()
    with pytest.raises(ValueError, match="contiguous float32"):
        env.observe_wide_sorted_device(buf[:7], OM)
    env.synchronize()
    assert bool((buf == -5.0).all())
    want = composed(env, OM)[0]
    out = torch.full((env.E, env.R, env.T + OM.width), -5.0, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        env.use_torch_stream()
        env.observe_wide_sorted_device(out, OM)
        side.synchronize()
        out.fill_(-5.0)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError, match="captured") as ei:
                env.observe_wide_sorted_device(out, OM)
            assert ei.value.code == _abi.ERR_UNSUPPORTED
        finally:
            graph.capture_end()
        side.synchronize()
        assert bool((out == -5.0).all())
        env.observe_wide_sorted_device(out, OM)
        side.synchronize()
    env.use_torch_stream()
    same(out.cpu().numpy(), want, "after the capture")
    env.close()


# ---------------------------------------------------------------------- 2. ebc_lstm_grad on wide rows
_nets = {}


def device_net(ni):
    """(net, state_dict, packed image by the header's pack, LstmNet on the device) of a seeded wide network, once."""
    if ni not in _nets:
        from ebcsim.lstm_train import LstmNet
        sd = lg.random_state_dict(oc.GRAD_NETS[ni], scale=4.0 if oc.GRAD_NETS[ni][0][5] == 7 else 1.0)
        _nets[ni] = (oc.GRAD_NETS[ni], sd, lg.host_pack(sd), LstmNet(sd, 0))
    return _nets[ni]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_grad(net, rows, target, nv, mask, scale):
    """(grad, loss_sum, count, value, joint) of one ebc_lstm_grad on host arrays, every output poisoned before."""
    B = rows.shape[0]
    grad = torch.full((net.packed_floats(),), -7.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -7.0, dtype=torch.float64, device=DEV), torch.full((), -7, dtype=torch.int64, device=DEV)
    value, joint = torch.full((B,), -7.0, dtype=torch.float32, device=DEV), torch.full((B, net.joint_dim), -7.0, dtype=torch.float32, device=DEV)
    net.grad(_dev(rows), _dev(target), grad, loss, count, scale, _dev(nv), _dev(mask), value, joint)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), joint.cpu().numpy()


def assert_same(got, want, tag):
    assert lg.same_bytes(got[0], want[0]), (tag, "grad", np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (tag, "loss_sum", got[1], want[1])
    assert got[2] == want[2], (tag, "count", got[2], want[2])
    assert lg.same_bytes(got[3], want[3]), (tag, "value", got[3], want[3])
    assert lg.same_bytes(got[4], want[4]), (tag, "joint", got[4], want[4])


@pytest.mark.parametrize("ni", range(len(oc.GRAD_NETS)), ids=oc.GRAD_IDS)
def test_wide_grad_kernel_equals_host_build_bytes(ni):
    """Rows 61 and 64 wide, narrow and reference widths, with mlp1 and without: at R = 1, 5 and ebc_lstm_net_grad_max_rows
    (11 with mlp1 and 23 without at the reference widths with 61 columns) and B in 1, C - 1, C, C + 1, 2 C + 1 (at the largest
    R: 1 and C + 1) grad, loss_sum, count, value and joint are the host build's, byte for byte,
    on plain batches and on the edge batches with n_valid and a mask; the packed image on the device is the header's."""
    net, sd, P, dn = device_net(ni)
    narrow = net[0][5] == 7
    image = torch.empty(dn.packed_floats(), dtype=torch.float32, device=DEV)
    assert lg.same_bytes(dn.get_packed(image).cpu().numpy(), P) and dn.widths[0] == net[0][0]
    R_max = dn.grad_max_rows()
    print("%s: ebc_lstm_net_grad_max_rows = %d" % (oc.GRAD_IDS[ni], R_max))
    if not narrow and net[0][0] == 61:
        assert R_max == oc.REFERENCE_MAX_ROWS[net[2]]
    assert R_max >= 10
    for R in (1, 5, R_max):
        for B in (lg.batches() if R <= 5 else [1, lg.chunk() + 1]):
            rows, target = lg.plain_batch(net, B, R)
            assert_same(kernel_grad(dn, rows, target, None, None, 2.0 / B), lg.host_grad(P, net, rows, target, None, None, 2.0 / B), ("plain", B, R))
            rows, target, nv, mask, kinds = lg.edge_batch(net, B, R)
            assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), lg.host_grad(P, net, rows, target, nv, mask, 2.0 / B), ("edge", B, R, kinds))
    if not narrow:  # one more row than the entry takes is refused by name, nothing written
        grad = torch.full((dn.packed_floats(),), -5.0, dtype=torch.float32, device=DEV)
        loss, count = torch.full((), -5.0, dtype=torch.float64, device=DEV), torch.full((), -5, dtype=torch.int64, device=DEV)
        with pytest.raises(_capi.EbcError) as err:
            dn.grad(torch.zeros((2, R_max + 1, net[0][0]), dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV), grad, loss, count, 1.0)
        assert err.value.code == _abi.ERR_UNSUPPORTED and "R = %d" % (R_max + 1) in str(err.value)
        torch.cuda.synchronize()
        assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5


def test_all_edge_kinds_were_covered():
    seen = set()
    for R in (1, 5):
        for B in lg.BATCHES:
            seen.update(lg.edge_batch(oc.GRAD_NETS[0], B, R)[4])
    assert seen == set(lg.EDGE_KINDS)


@pytest.mark.parametrize("case", oc.kernel_accuracy_cases(), ids=oc.case_name)
def test_wide_grad_kernel_against_float64_autograd(case):
    """Per parameter tensor and for the loss: the kernel's error against float64 autograd of LstmModule is within 8 x torch's
    own float32 error, floored at 2^-25."""
    from ebcsim.lstm_train import LstmNet
    ref = oc.reference_of(case)
    dn = LstmNet(ref["sd"], 0)
    g, loss, count, _, _ = kernel_grad(dn, ref["rows"], ref["target"], None, None, ref["scale"])
    assert count == ref["rows"].shape[0]
    tensors, lrow = oc.accuracy_of(case, g, loss)
    for key, er, et, bar in tensors + [("loss_sum",) + lrow]:
        print("%-34s %-22s kernel %.3e torch32 %.3e bar %.3e" % (oc.case_name(case), key, er, et, bar))
    for key, er, et, bar in tensors + [("loss_sum",) + lrow]:
        assert er <= bar, (key, er, et, bar)


# ---------------------------------------------------------------------- 3. decisions
@pytest.mark.parametrize("name", oc.RUNS)
def test_om_lstm_decisions_gpu(name):
    """The recorded run on one env, DeviceSarlPolicy(LstmValueNet 61 wide, om=spec) deciding: the reference's action at EVERY
    decision, every recorded value within F_CELL x e_ref (LstmModule float32 against its float64 copy on the wide rows of
    the decision, measured here), the recorded infos and rewards; every forward ran in the library."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.lstm_rl import LstmValueNet
    from ebcsim.sarl import DeviceSarlPolicy
    z, meta, spec, m32, m64 = oc.golden_run(name)
    b = batch_from_init(z, copies=1)
    env = BatchedEnv(params_of(z), 1, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = LstmValueNet(oc.golden_state_dict(meta), device=DEV)
    assert net.input_dim == env.T + spec.width == 61
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"], om=spec)
    outs = env.alloc_step_outputs(("reward", "done", "info"))
    steps = len(z["action"])
    e_ref, errs = 0.0, []
    for t in range(steps):
        actions, values = pol.decide(env)
        torch.cuda.synchronize()
        v = values.cpu().numpy()
        e_ref = max(e_ref, oc.value_error(m32, m64, pol._wide[0]))
        errs.append(float(np.abs(v[0] - z["values"][t]).max()))
        assert int(np.argmax(v[0])) == oc.chosen_index(z, t), "decision %d" % t
        np.testing.assert_array_equal(actions.cpu().numpy(), z["action"][t][None], err_msg="decision %d" % t)
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_CACHED)
        torch.cuda.synchronize()
        assert int(outs["info"][0]) == int(z["info"][t]), t
        np.testing.assert_allclose(float(outs["reward"][0]), z["reward"][t], atol=1e-9)
    tol = F_CELL * e_ref
    print("%s: %d decisions, e_ref %.3g, tolerance %.3g, |values - recorded| %.3g, top-2 gap %.3g" % (name, steps, e_ref, tol, max(errs), meta["top2_gap"]))
    assert max(errs) <= tol, (max(errs), tol)
    assert int(z["info"][-1]) == int(meta["final_info"])
    assert net._native_blocks() is not None and net.native_forwards >= steps


def test_value_net_refuses_rows_wider_than_64_by_name():
    from ebcsim.lstm_rl import LstmValueNet
    net = LstmValueNet(lg.random_state_dict(oc.wide(lg.NARROW_NET1, 65)), device=DEV)
    with pytest.raises(NotImplementedError, match="up to 64 wide"):
        net.forward(torch.zeros((2, 3, 65), dtype=torch.float32, device=DEV))
    assert net.native_forwards == 0


# ---------------------------------------------------------------------- 4. collect
def collect_envs(n, seed=6400, E=8):
    return [make_env(params_for(13), scenes(seed, E, RAGGED, goal=(0.1, 1.2)), scenes(seed + 1, 2 * E, RAGGED[1:] + RAGGED[:1], goal=(0.3, 1.2)))
            for _ in range(n)]


def memory_bytes(m):
    n = len(m)
    return m.states[:n].cpu().numpy(), m.values[:n].cpu().numpy(), m.n_valid[:n].cpu().numpy(), m.position, m.ragged


def same_memory(a, b, tag):
    ma, mb = memory_bytes(a), memory_bytes(b)
    assert len(a) == len(b) > 0 and ma[3:] == mb[3:], (tag, len(a), len(b))
    for x, y, name in zip(ma[:3], mb[:3], ("states", "values", "n_valid")):
        same(x, y, (tag, name))


def composed_collect(env, policy, target_net, memory, steps, om):
    """collect (epsilon 0, no episode store) from the existing entries.  With a spec: the stored state and the next state
    are observe_wide_sorted_composed after each step.  Without: the parent's LSTM-RL loop, ebc_observe's rotated rows and
    the step's obs_rotated through sort_rows_by_distance."""
    from ebcsim.lstm_train import sort_rows_by_distance
    from ebcsim.sarl import uniform_v_pref
    from ebcsim.train import value_targets
    gamma_bar = GAMMA ** (env.params.time_step * uniform_v_pref(env))
    outs = env.alloc_step_outputs(("reward", "done", "info", "obs_rotated"))

    def state():
        if om is not None:
            return observe_wide_sorted_composed(env, om)
        s = torch.empty((env.E, env.R, env.T), dtype=torch.float32, device=DEV)
        env.observe_device(s)
        return s
    cur = state()
    for _ in range(steps):
        actions, _ = policy.decide(env)
        nv = policy.n_valid.clone()
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_CACHED, flags=AUTO)
        if om is not None:
            nxt, kept = state(), cur
        else:
            nxt, kept = sort_rows_by_distance(outs["obs_rotated"], nv), sort_rows_by_distance(cur, nv)
        memory.push(kept.clone(), value_targets(outs["reward"], outs["done"], nxt, target_net, gamma_bar, nv), nv)
        cur = state()
    env.synchronize()


@pytest.mark.parametrize("om", [OM, None], ids=["om_sorted", "parent"])
def test_collect_fills_the_memory_of_the_composition(om):
    """8 envs, 4 greedy decisions of DeviceSarlPolicy over LstmValueNet.  collect(om=spec, sorted_rows=True): the replay is the
    composition's, byte for byte — the stored state and the next state the target network values are
    observe_wide_sorted_composed after each step.  collect without the new arguments (LSTM-RL's state_transform): the
    parent's loop's bytes."""
    from ebcsim.actions import build_action_space
    from ebcsim.lstm_rl import LstmValueNet
    from ebcsim.lstm_train import sort_rows_by_distance
    from ebcsim.sarl import DeviceSarlPolicy
    from ebcsim.train import DeviceReplay, collect
    a, b = collect_envs(2)
    W = 0 if om is None else om.width
    net = LstmValueNet(lg.random_state_dict(oc.wide(lg.REFERENCE_NET2, 13 + W)), device=DEV)
    space = build_action_space(0.7)
    kw = {} if om is None else {"om": om}
    pa, pb = DeviceSarlPolicy(net, space, GAMMA, **kw), DeviceSarlPolicy(net, space, GAMMA, **kw)
    ma, mb = DeviceReplay(4096, a.R, a.T + W, DEV), DeviceReplay(4096, b.R, b.T + W, DEV)
    if om is None:
        mean_r = collect(a, pa, net, ma, 4, GAMMA, state_transform=sort_rows_by_distance)
    else:
        mean_r = collect(a, pa, net, ma, 4, GAMMA, om=om, sorted_rows=True)
    composed_collect(b, pb, net, mb, 4, om)
    assert np.isfinite(mean_r) and len(ma) == 32
    same_memory(ma, mb, "collect")
    assert bool(torch.isfinite(ma.values[:32]).all()) and ma.ragged
    st = ma.states[:32].cpu().numpy()
    nv = ma.n_valid[:32].cpu().numpy()
    for i in range(32):
        assert (np.diff(st[i, :nv[i], 11]) <= 0).all()  # stored in decreasing distance
    if om is not None:
        assert st[:, :, 13:].any()
        with pytest.raises(ValueError, match="sorted_rows needs om"):
            collect(a, pa, net, ma, 1, GAMMA, sorted_rows=True)
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        same(sa[key], sb[key], "state " + key)
    a.close()
    b.close()


# ---------------------------------------------------------------------- 5. the schedule
def test_om_lstm_schedule_end_to_end(tmp_path):
    """Tiny: 16 envs of goals within the robot's radius plus one step (every episode ends at its first step, so the replay
    fills), 2 imitation steps and 1 epoch, 2 RL rounds on the 61-wide ValueNetwork2: the losses are finite, the weights
    changed in both stages (the map columns too), the saved files load into LstmModule at width 61 with strict=True, and a
    row count above ebc_lstm_net_grad_max_rows is refused by name."""
    from ebcsim.actions import build_action_space
    from ebcsim.batched import BatchedEnv
    from ebcsim.lstm_rl import LstmModule
    from ebcsim.lstm_train import LstmTrainer, run_lstm_training
    E = 16
    env = make_env(params_for(13), scenes(6500, E, RAGGED, goal=(0.05, 0.12)), scenes(6501, 4 * E, RAGGED[2:] + RAGGED[:2], goal=(0.05, 0.12)))
    net_shape = oc.wide(lg.REFERENCE_NET2, 61)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        tr = LstmTrainer(lg.module(net_shape), device=DEV, optimizer="sgd", lr=0.01)
    assert tr.native and tr.widths[0] == 61 and tr.net.grad_max_rows() == oc.REFERENCE_MAX_ROWS[True]
    start = tr.state_dict()
    space = build_action_space(0.7)
    with pytest.raises(NotImplementedError, match="the network takes 61"):
        run_lstm_training(env, tr, space, GAMMA, il_steps=1)
    big = BatchedEnv(params_for(13), 2, 11, 1)
    with pytest.raises(NotImplementedError, match="12 rows per state, ebc_lstm_grad takes 11 for this network; use native=False"):
        run_lstm_training(big, tr, space, GAMMA, il_steps=1, om=OM)
    big.close()
    hist = run_lstm_training(env, tr, space, GAMMA, il_steps=2, il_epochs=1, train_iterations=2, steps_per_iteration=2, train_batches=2,
                             batch_size=16, capacity=4096, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=1,
                             generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path), om=OM)
    torch.cuda.synchronize()
    print(hist)
    assert hist["il_stored"] > 0 and hist["il_loss"] is not None and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 2 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["native_refreshes"] == 2 and hist["native_forwards"] > 0 and hist["memory"] > hist["il_stored"]
    files = {}
    for name in ("il_model.pth", "rl_model_2.pth"):
        files[name] = torch.load(str(tmp_path / name), map_location="cpu")
        m = LstmModule.from_state_dict(files[name])
        assert m.input_dim == 61 and m.with_interaction_module and tuple(files[name]["mlp1.0.weight"].shape) == (150, 61)
        lg.module(net_shape).load_state_dict(files[name], strict=True)
        assert all(bool(torch.isfinite(v).all()) for v in files[name].values())
    assert not all(torch.equal(files["il_model.pth"][k], start[k]) for k in start)
    assert not all(torch.equal(files["rl_model_2.pth"][k], files["il_model.pth"][k]) for k in start)
    assert not torch.equal(files["rl_model_2.pth"]["mlp1.0.weight"][:, 13:], start["mlp1.0.weight"][:, 13:])  # the map columns learn
    env.close()
