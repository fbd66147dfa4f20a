"""Training OM-SARL on the device: ebc_observe_wide against the four-call composition it replaces, byte for byte;
ebc_step_k_om against ebc_step_k on a twin handle and against ebc_observe_wide between single steps; ebc_sarl_grad on the
networks of ebc_sarl_net_create_om against the host build of the rule on wide rows, byte for byte; collect_il and collect
with a spec against a composition of the existing entries, and without one against the parent's code path; the schedule
end to end.  Cases and the bars: tests/om_train_cases.py."""
import configparser
import ctypes as C
import os

import numpy as np
import pytest
import torch

import om_train_cases as oc
import sarl_grad_cases as sg
from sail_rollout_cases import params_for
from ebcsim import _abi, _capi, scene as ebc_scene
from ebcsim.occupancy import OccupancySpec, observe_wide_composed, wide_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = oc.ROOT
AUTO = _abi.FLAG_AUTO_RESET
SPECS = [OccupancySpec(n, {1: 3.0, 4: 1.0}[n], c) for c in (1, 2, 3) for n in (1, 4)]
# (humans, static rows) per scene: 1, 2, 3, 4 and 2 observation rows
RAGGED = [(1, 0), (1, 1), (2, 1), (3, 1), (2, 0), (3, 0), (1, 1), (3, 1)]


def scenes(seed, E, counts, N=3, S=1, goal=(0.1, 1.5)):
    """E scenes of N human and S static slots of which scene e uses counts[e % len(counts)]; the robot's goal lies
    goal[0] .. goal[1] ahead of it (scene 0: goal[0], an episode that ends at its first step); unused slots are zeros."""
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


def ragged_env(T, kin, E=5, seed=4100):
    return make_env(params_for(T, kin), scenes(seed, E, RAGGED), scenes(seed + 1, 2 * E, RAGGED[3:] + RAGGED[:3]))


def same(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8), err_msg=str(tag))


def observe_wide(env, spec, with_rows=True, fill=-7.0):
    out = torch.full((env.E, env.R, env.T + spec.width), fill, dtype=torch.float32, device=DEV)
    n = torch.full((env.E,), -7, dtype=torch.int64, device=DEV) if with_rows else None
    env.observe_wide_device(out, spec, n)
    env.synchronize()
    return out.cpu().numpy(), None if n is None else n.cpu().numpy()


def composed(env, spec):
    n = torch.full((env.E,), -7, dtype=torch.int64, device=DEV)
    wide = observe_wide_composed(env, spec, n_rows=n)
    env.synchronize()
    return wide.cpu().numpy(), n.cpu().numpy()


# ---------------------------------------------------------------------- 1. ebc_observe_wide
@pytest.mark.parametrize("kin", [_abi.HOLONOMIC, _abi.UNICYCLE], ids=["holonomic", "unicycle"])
@pytest.mark.parametrize("T", [13, 17])
def test_observe_wide_is_the_four_call_composition_in_bytes(T, kin):
    """5 envs of 3 human + 1 static slots, row counts 1 .. 4, a ragged pool; channels 1, 2, 3 x cell_num 1 and 4, at the
    reset state and after two steps with restarts: state_wide and n_rows are the bytes of ebc_observe (rotated) |
    ebc_occupancy_rows on ebc_observe's ob with ebc_row_counts, and the numpy path's on the same inputs."""
    env = ragged_env(T, kin)
    act = np.tile([0.4, 0.2], (env.E, 1))
    for visit in range(3):
        counts = env.row_counts()
        if visit == 0:
            assert sorted(counts.tolist()) == [1, 2, 2, 3, 4] and env.ragged
        ob, rot = env.observe()
        for spec in SPECS:
            got, n = observe_wide(env, spec)
            want, wn = composed(env, spec)
            same(got, want, (visit, spec))
            same(n, wn, (visit, spec, "n_rows"))
            same(n, counts, (visit, spec, "row_counts"))
            same(got, wide_state(rot, ob, counts, spec), (visit, spec, "numpy"))
            assert not got[np.arange(env.R)[None, :] >= counts[:, None]].any()  # padding: zero rows, zero maps
            same(observe_wide(env, spec, with_rows=False)[0], want, (visit, spec, "no n_rows"))
        if visit == 0:
            assert any(observe_wide(env, s)[0][:, :, T:].any() for s in SPECS)  # some map is not empty
        done = env.step(robot_action=act, human_policy=_abi.HUMAN_ORCA, flags=AUTO)["done"]
        assert visit > 0 or done[0]  # env 0 ends at its first step and restarts from the pool
    env.close()


def test_observe_wide_at_the_lds_limit():
    """R = 128 (33 human + 95 static slots), W = 192 (cell_num 8, 3 channels), T = 17, E = 2, the second env ragged."""
    b = scenes(4200, 2, [(33, 95), (20, 50)], N=33, S=95)
    env = make_env(params_for(17), b)
    spec = OccupancySpec(8, 1.0, 3)
    assert env.R == 128 and spec.width == 192
    got, n = observe_wide(env, spec)
    want, wn = composed(env, spec)
    same(got, want, "limit")
    same(n, wn, "limit n_rows")
    assert n.tolist() == [128, 70] and got[:, :, 17:].any() and not got[1, 70:].any()
    env.close()


def test_observe_wide_refusals_and_capture():
    """channels outside {1, 2, 3}, cell_num 0, a cell_size that is not a finite positive number, W > 192, NULL output,
    a bad struct_size, before ebc_reset, a capturing stream: refused by name with nothing written; usable afterwards."""
    from ebcsim.batched import BatchedEnv
    lib = _capi.lib()
    params = params_for(17)
    raw = BatchedEnv(params, 2, 3, 1)
    buf = torch.full((4096,), -5.0, dtype=torch.float32, device=DEV)
    good = _abi.om_spec(OccupancySpec(4, 1.0, 3))
    assert lib.ebc_observe_wide(raw._h, C.addressof(good), buf.data_ptr(), None) == _abi.ERR_STATE and b"before ebc_reset" in lib.ebc_last_error()
    raw.close()
    env = ragged_env(17, _abi.HOLONOMIC)
    for change, word in ((dict(channels=0), b"channels"), (dict(channels=4), b"channels"), (dict(cell_num=0), b"cell_num < 1"),
                         (dict(cell_num=9), b"W > 192"), (dict(cell_size=0.0), b"cell_size"), (dict(cell_size=-1.0), b"cell_size"),
                         (dict(cell_size=float("inf")), b"cell_size"), (dict(cell_size=float("nan")), b"cell_size")):
        s = _abi.om_spec(OccupancySpec(4, 1.0, 3))
        for k, v in change.items():
            setattr(s, k, v)
        assert lib.ebc_observe_wide(env._h, C.addressof(s), buf.data_ptr(), None) == _abi.ERR_UNSUPPORTED, change
        assert word in lib.ebc_last_error() and b"ebc_observe_wide" in lib.ebc_last_error(), (change, lib.ebc_last_error())
    assert lib.ebc_observe_wide(env._h, C.addressof(good), None, None) == _abi.ERR_INVALID and b"state_wide is NULL" in lib.ebc_last_error()
    short = _abi.om_spec(OccupancySpec(4, 1.0, 3))
    short.struct_size -= 4
    assert lib.ebc_observe_wide(env._h, C.addressof(short), buf.data_ptr(), None) == _abi.ERR_INVALID and b"EbcOmSpec.struct_size" in lib.ebc_last_error()
    env.synchronize()
    assert bool((buf == -5.0).all())
    spec = OccupancySpec(4, 1.0, 3)
    want = composed(env, spec)[0]
    out = torch.full((env.E, env.R, env.T + spec.width), -5.0, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        env.use_torch_stream()
        env.observe_wide_device(out, spec)
        side.synchronize()
        out.fill_(-5.0)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError, match="captured") as ei:
                env.observe_wide_device(out, spec)
            assert ei.value.code == _abi.ERR_UNSUPPORTED
        finally:
            graph.capture_end()
        side.synchronize()
        assert bool((out == -5.0).all())
        env.observe_wide_device(out, spec)
        side.synchronize()
    env.use_torch_stream()
    same(out.cpu().numpy(), want, "after the capture")
    env.close()


# ---------------------------------------------------------------------- 2. ebc_step_k_om
STEP_K_KEYS = ("state_rotated", "n_rows", "robot_action_out", "reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated")


@pytest.mark.parametrize("T", [13, 17])
def test_step_k_om_is_step_k_plus_the_wide_states(T):
    """K = 6 on 4 envs, the robot on ORCA, auto-reset over a ragged pool, env 0 arriving at its first step: every output of
    EbcStepKArgs is ebc_step_k's on a twin handle, state_wide[k] is observe_wide_device taken between K single steps on a
    third, and the three handles end in the same state."""
    K, E, spec = 6, 4, OccupancySpec(4, 1.0, 3)
    envs = [make_env(params_for(T), scenes(4300, E, RAGGED), scenes(4301, 2 * E, RAGGED[2:] + RAGGED[:2])) for _ in range(3)]
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, flags=AUTO, robot_safety_space=0.15)
    a = envs[0].alloc_step_k_outputs(K, STEP_K_KEYS + ("state_wide",), om=spec)
    assert tuple(a["state_wide"].shape) == (K, E, envs[0].R, T + spec.width)
    a["state_wide"].fill_(-7.0)
    envs[0].step_k_device(a, K, om=spec, **kw)
    b = envs[1].alloc_step_k_outputs(K, STEP_K_KEYS)
    envs[1].step_k_device(b, K, **kw)
    singles = []
    c = envs[2].alloc_step_k_outputs(1, ("done",))
    for k in range(K):
        singles.append(observe_wide(envs[2], spec)[0])
        envs[2].step_k_device(c, 1, **kw)
    for e in envs:
        e.synchronize()
    assert a["done"].cpu().numpy()[:, 0].any() and a["done"].cpu().numpy().sum() >= 1  # an episode ended inside the window
    for key in STEP_K_KEYS:
        same(a[key].cpu().numpy(), b[key].cpu().numpy(), key)
    wide = a["state_wide"].cpu().numpy()
    same(wide, np.stack(singles), "state_wide")
    same(wide[:, :, :, :T], a["state_rotated"].cpu().numpy(), "the rotated columns")
    assert wide[:, :, :, T:].any()
    for other in envs[1:]:
        sa, sb = envs[0].get_state(), other.get_state()
        for key in sa:
            same(sa[key], sb[key], "state " + key)
    # the one-launch form is refused by name, and so is a spec outside the limits; the handle goes on
    with pytest.raises(_capi.EbcError, match="ebc_step_k_om: EBC_FLAG_ONE_LAUNCH") as ei:
        envs[0].step_k_device(a, K, om=spec, **dict(kw, flags=AUTO | _abi.FLAG_ONE_LAUNCH))
    assert ei.value.code == _abi.ERR_UNSUPPORTED
    with pytest.raises(_capi.EbcError, match="ebc_step_k_om: W > 192") as ei:
        envs[0].step_k_device(dict(a, state_wide=torch.zeros((K, E, envs[0].R, T + 243), dtype=torch.float32, device=DEV)), K,
                              om=OccupancySpec(9, 1.0, 3), **kw)
    assert ei.value.code == _abi.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="go together"):
        envs[0].step_k_device(b, K, om=spec, **kw)
    envs[0].step_k_device(a, K, om=spec, **kw)
    envs[1].step_k_device(b, K, **kw)
    envs[0].synchronize()
    envs[1].synchronize()
    same(a["reward"].cpu().numpy(), b["reward"].cpu().numpy(), "the next window")
    for e in envs:
        e.close()


# ---------------------------------------------------------------------- 3. ebc_sarl_grad on wide networks
_nets = {}


def device_net(wnet):
    """(state_dict, packed image by the header's pack, SarlNet by ebc_sarl_net_create_om) of a seeded wide network, once."""
    key = (tuple(wnet[0][0]), wnet[0][1], wnet[0][2], wnet[1])
    if key not in _nets:
        from ebcsim.sarl_train import SarlNet
        sd = sg.random_state_dict(wnet[0])
        _nets[key] = (sd, oc.host_pack(sd, wnet[1]), SarlNet(sd, 0, om_width=wnet[1]))
    return _nets[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_grad(net, rows, target, nv, mask, scale, fill=-7.0):
    B, R, _ = rows.shape
    grad = torch.full((net.packed_floats(),), fill, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), fill, dtype=torch.float64, device=DEV), torch.full((), -7, dtype=torch.int64, device=DEV)
    value, att = torch.full((B,), fill, dtype=torch.float32, device=DEV), torch.full((B, R), fill, dtype=torch.float32, device=DEV)
    net.grad(_dev(rows), _dev(target), grad, loss, count, scale, _dev(nv), _dev(mask), value, att)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), att.cpu().numpy()


def assert_same(got, want, tag):
    assert oc.same_bytes(got[0], want[0]), (tag, "grad", np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (tag, "loss_sum", got[1], want[1])
    assert got[2] == want[2], (tag, "count", got[2], want[2])
    assert oc.same_bytes(got[3], want[3]), (tag, "value", got[3], want[3])
    assert oc.same_bytes(got[4], want[4]), (tag, "attention", got[4], want[4])


@pytest.mark.parametrize("wi", [0, 1, 2], ids=["61", "65", "224"])
def test_wide_kernel_equals_host_build_bytes(wi):
    """B in 1, 3, 4, 5, 9 at the narrow hidden widths with T + W = 61, 65, 224 (R = 3, and R = 1 and 5 at B = 5): grad,
    loss_sum, count, value and attention are the host build's, byte for byte, on wide batches with ragged n_valid and a
    mask, and on the edge batches of tests/sarl_grad_cases.py; the packed image on the device is the header's."""
    wnet = oc.NARROW_WIDE[wi]
    sd, P, dn = device_net(wnet)
    assert dn.widths[0] == wnet[0][0][0] and dn.packed_floats() == len(P)
    image = torch.empty(dn.packed_floats(), dtype=torch.float32, device=DEV)
    assert oc.same_bytes(dn.get_packed(image).cpu().numpy(), P)
    for B, R in [(B, 3) for B in oc.BATCHES] + [(5, 1), (5, 5)]:
        rows, target = oc.wide_batch(wnet, B, R, seed=5000 + 100 * wi + 10 * B + R)
        nv, mask = oc.ragged_masked(B, R, seed=5001 + B + R)
        assert_same(kernel_grad(dn, rows, target, None, None, 2.0 / B), oc.host_grad(P, wnet, rows, target, None, None, 2.0 / B), ("plain", B, R))
        assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), oc.host_grad(P, wnet, rows, target, nv, mask, 2.0 / B), ("ragged", B, R))
        rows, target, nv, mask, kinds = sg.edge_batch(wnet[0], B, R)
        assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), oc.host_grad(P, wnet, rows, target, nv, mask, 2.0 / B), ("edge", B, R, kinds))


def test_wide_kernel_at_the_reference_widths_and_its_largest_r():
    """The reference widths with T + W = 17 + 48: the host build's bytes at B = 5, R = 5; ebc_sarl_net_grad_max_rows answers
    for the wide slot (68 floats of X, not 20: fewer rows than the plain network takes), R = that runs and gives the host
    build's bytes, R + 1 is EBC_ERR_UNSUPPORTED with every output left as it was."""
    wnet = oc.REFERENCE_WIDE_65
    sd, P, dn = device_net(wnet)
    rows, target = oc.wide_batch(wnet, 5, 5, seed=5300)
    nv, mask = oc.ragged_masked(5, 5, seed=5301)
    assert_same(kernel_grad(dn, rows, target, nv, mask, 0.4), oc.host_grad(P, wnet, rows, target, nv, mask, 0.4), "reference 65")
    R = dn.grad_max_rows()
    slot, state = 68 + 152 + 100 + 100 + 52 + 100 + 100 + 2, 100 + 56 + 52 + 152 + 100 + 100 + 6
    assert 4 * 4 * (R * slot + state) <= 160 * 1024 < 4 * 4 * ((R + 1) * slot + state) and R >= 10
    B = sg.chunk() + 1
    rows, target = oc.wide_batch(wnet, B, R, seed=5302)
    nv = np.array([R, 1, R + 3, R - 1, R][:B], dtype=np.int64)
    assert_same(kernel_grad(dn, rows, target, nv, None, 0.4), oc.host_grad(P, wnet, rows, target, nv, None, 0.4), "largest R")
    grad = torch.full((dn.packed_floats(),), -5.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -5.0, dtype=torch.float64, device=DEV), torch.full((), -5, dtype=torch.int64, device=DEV)
    value, att = torch.full((2,), -5.0, dtype=torch.float32, device=DEV), torch.full((2, R + 1), -5.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_capi.EbcError) as err:
        dn.grad(torch.zeros((2, R + 1, 65), dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV), grad, loss, count, 1.0,
                value=value, attention=att)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "LDS" in str(err.value) and "R = %d" % (R + 1) in str(err.value)
    with pytest.raises(_capi.EbcError) as err:  # the rotated width alone is not what this network takes
        dn.grad(torch.zeros((2, 2, 17), dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV), grad, loss, count, 1.0)
    assert err.value.code == _abi.ERR_INVALID and "17 wide, the network takes 65" in str(err.value)
    torch.cuda.synchronize()
    assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5 and bool((value == -5.0).all()) and bool((att == -5.0).all())


def test_om_width_zero_is_the_plain_network():
    from ebcsim.sarl_train import SarlNet
    net = sg.NARROW_T17_NET
    sd = sg.random_state_dict(net)
    plain, zero = SarlNet(sd, 0), SarlNet(sd, 0, om_width=0)
    assert plain.packed_floats() == zero.packed_floats() and plain.grad_max_rows() == zero.grad_max_rows() and plain.widths == zero.widths
    a, b = (torch.empty(n.packed_floats(), dtype=torch.float32, device=DEV) for n in (plain, zero))
    assert torch.equal(plain.get_packed(a), zero.get_packed(b))
    rows, target, nv, mask, _ = sg.edge_batch(net, 9, 5)
    assert_same(kernel_grad(zero, rows, target, nv, mask, 0.2), kernel_grad(plain, rows, target, nv, mask, 0.2), "om_width 0")
    assert_same(kernel_grad(zero, rows, target, nv, mask, 0.2), sg.host_grad(sg.host_pack(sd), net, rows, target, nv, mask, 0.2), "host")


# ---------------------------------------------------------------------- 4. collect_il and collect
GAMMA = 0.9
OM = OccupancySpec(4, 1.0, 3)


def collect_envs(n, seed=4400, E=8):
    return [make_env(params_for(17), scenes(seed, E, RAGGED, goal=(0.1, 1.2)), scenes(seed + 1, 2 * E, RAGGED[1:] + RAGGED[:1], goal=(0.3, 1.2)))
            for _ in range(n)]


def wide_value_net():
    from ebcsim.sarl import SarlValueNet
    sd = sg.random_state_dict(oc.REFERENCE_WIDE_65[0])
    return SarlValueNet(sd, device=DEV)


def plain_value_net():
    from ebcsim.sarl import SarlValueNet
    return SarlValueNet(sg.random_state_dict(([17] + oc.REFERENCE_UNITS, 6, True)), device=DEV)


def memory_bytes(m):
    n = len(m)
    return m.states[:n].cpu().numpy(), m.values[:n].cpu().numpy(), m.n_valid[:n].cpu().numpy(), m.position, m.ragged


def same_memory(a, b, tag):
    ma, mb = memory_bytes(a), memory_bytes(b)
    assert len(a) == len(b) > 0 and ma[3:] == mb[3:], (tag, len(a), len(b))
    for x, y, name in zip(ma[:3], mb[:3], ("states", "values", "n_valid")):
        same(x, y, (tag, name))


def composed_collect_il(env, memory, steps, om):
    """collect_il from the existing entries: per step the state (rotated, or the four-call wide one), the row counts and
    one ebc_step_k of a single step with the robot on ORCA; then the targets of the window."""
    from ebcsim.train import il_value_targets
    from ebcsim.sarl import uniform_v_pref
    env.robot_orca_sim(True)
    gamma_bar = GAMMA ** (env.params.time_step * uniform_v_pref(env))
    states, rows, outs = [], [], {k: [] for k in ("reward", "done", "info")}
    for _ in range(steps):
        if om is None:
            s = torch.empty((env.E, env.R, env.T), dtype=torch.float32, device=DEV)
            env.observe_device(s)
        else:
            s = observe_wide_composed(env, om)
        n = torch.empty((env.E,), dtype=torch.int64, device=DEV)
        env.row_counts_device(n)
        o = env.alloc_step_k_outputs(1, ("reward", "done", "info"))
        env.step_k_device(o, 1, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, flags=AUTO, robot_safety_space=0.15)
        states.append(s)
        rows.append(n)
        for k in outs:
            outs[k].append(o[k][0])
    states, rows = torch.stack(states), torch.stack(rows)
    values, keep = il_value_targets(torch.stack(outs["reward"]), torch.stack(outs["done"]), gamma_bar, torch.stack(outs["info"]))
    keep = keep.reshape(-1)
    memory.push(states.reshape(-1, env.R, states.shape[-1])[keep], values.reshape(-1)[keep], rows.reshape(-1)[keep])
    env.synchronize()
    return int(keep.sum())


def composed_collect(env, policy, target_net, memory, steps, om):
    """collect (epsilon 0, no episode store) from the existing entries: the parent's loop, the states taken with
    ebc_observe (om None) or with the four-call composition."""
    from ebcsim.train import value_targets
    from ebcsim.sarl import uniform_v_pref
    gamma_bar = GAMMA ** (env.params.time_step * uniform_v_pref(env))
    outs = env.alloc_step_outputs(("reward", "done", "info", "obs_rotated"))

    def state():
        if om is not None:
            return observe_wide_composed(env, om)
        s = torch.empty((env.E, env.R, env.T), dtype=torch.float32, device=DEV)
        env.observe_device(s)
        return s
    cur = state()
    for _ in range(steps):
        actions, _ = policy.decide(env)
        nv = policy.n_valid.clone()
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_CACHED, flags=AUTO)
        nxt = outs["obs_rotated"] if om is None else state()
        memory.push(cur.clone(), value_targets(outs["reward"], outs["done"], nxt, target_net, gamma_bar, nv), nv)
        cur = state()
    env.synchronize()


@pytest.mark.parametrize("om", [OM, None], ids=["om", "no_om"])
def test_collect_il_fills_the_memory_of_the_composition(om):
    """8 envs, 12 steps, the robot on ORCA: with a spec the replay's states, values and row counts are the bytes of the
    composition of existing entries on a twin handle; with om=None those of the parent's code path (the same composition
    with ebc_observe's rotated rows): the new argument changes nothing there."""
    from ebcsim.train import DeviceReplay, collect_il
    a, b = collect_envs(2)
    W = 0 if om is None else om.width
    ma, mb = DeviceReplay(4096, a.R, a.T + W, DEV), DeviceReplay(4096, b.R, b.T + W, DEV)
    stored, ended = collect_il(a, ma, 12, GAMMA, safety_space=0.15) if om is None else collect_il(a, ma, 12, GAMMA, safety_space=0.15, om=om)
    assert stored == composed_collect_il(b, mb, 12, om) and stored > 0 and ended > 0 and len(ma) == stored
    same_memory(ma, mb, "collect_il")
    assert ma.ragged and len(set(ma.n_valid[:len(ma)].tolist())) > 1
    if om is not None:
        assert bool(ma.states[:len(ma), :, a.T:].any())
        with pytest.raises(_capi.EbcError, match="EBC_FLAG_ONE_LAUNCH"):
            collect_il(a, ma, 4, GAMMA, safety_space=0.15, om=om, one_launch=True)
    a.close()
    b.close()


@pytest.mark.parametrize("om", [OM, None], ids=["om", "no_om"])
def test_collect_fills_the_memory_of_the_composition(om):
    """8 envs, 6 greedy decisions of DeviceSarlPolicy (with the spec: the OM policy on the 65-wide network): the replay is
    the composition's, byte for byte — with a spec the stored state and the next state the target network values are
    ebc_observe | the maps of the current state; without one the parent's loop."""
    from ebcsim.actions import build_action_space
    from ebcsim.sarl import DeviceSarlPolicy
    from ebcsim.train import DeviceReplay, collect
    a, b = collect_envs(2, seed=4500)
    net = plain_value_net() if om is None else wide_value_net()
    space = build_action_space(0.7)
    kw = {} if om is None else {"om": om}
    pa, pb = DeviceSarlPolicy(net, space, GAMMA, **kw), DeviceSarlPolicy(net, space, GAMMA, **kw)
    W = 0 if om is None else om.width
    ma, mb = DeviceReplay(4096, a.R, a.T + W, DEV), DeviceReplay(4096, b.R, b.T + W, DEV)
    mean_r = collect(a, pa, net, ma, 6, GAMMA, **kw)
    composed_collect(b, pb, net, mb, 6, om)
    assert np.isfinite(mean_r) and len(ma) == 48
    same_memory(ma, mb, "collect")
    assert bool(torch.isfinite(ma.values[:48]).all())
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        same(sa[key], sb[key], "state " + key)
    a.close()
    b.close()


# ---------------------------------------------------------------------- 5. the schedule
def generated_env(E):
    """E envs of the five-adult config with the project's OM policy config on device-generated train scenes with a restart
    pool, as tools/train_sarl.py builds them."""
    from ebcsim import actions as ebc_actions, config as ebc_config
    from ebcsim.batched import BatchedEnv
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_om.config"))
    params = ebc_config.params_from_config(cfg, pol)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "train")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    seed0 = ebc_scene.COUNTER_OFFSET["train"]
    env.generate_reset(gen, seed0)
    env.generate_pool(gen, seed0 + E, 8 * E)
    return env, ebc_actions.build_action_space(sc.robot.v_pref), OccupancySpec.from_config(pol)


def test_training_schedule_with_maps_end_to_end(tmp_path):
    """What tools/train_sarl.py runs with policy_om.config, small: 64 envs, 40 imitation steps and 2 epochs, then 3 RL rounds
    of 4 optimizer steps on the 17 + 48 wide network: it ends, every loss and target is finite, the deciding blocks were
    refreshed every round, the saved files load strict into the wide SarlModule, and DeviceSarlPolicy(om=spec) decides
    with the refreshed weights: its values differ from the starting network's."""
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    from ebcsim.sarl_train import SarlTrainer, run_sarl_training
    env, space, om = generated_env(64)
    assert env.R == 5 and env.T == 17 and om == OM
    net_shape = ([65] + oc.REFERENCE_UNITS, 6, True)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        tr = SarlTrainer(sg.module(net_shape), device=DEV, optimizer="sgd", lr=0.01, om_width=om.width)
    assert tr.native and tr.net.om_width == 48 and tr.widths[0] == 65
    start = tr.state_dict()
    with pytest.raises(NotImplementedError, match="occupancy maps 0, the network takes 65"):
        run_sarl_training(env, tr, space, GAMMA, il_steps=1)
    probe = DeviceSarlPolicy(SarlValueNet(start, device=DEV), space, GAMMA, om=om)
    v0 = probe.decide(env)[1].clone()
    seen = []
    hist = run_sarl_training(env, tr, space, GAMMA, il_steps=40, il_epochs=2, train_iterations=3, steps_per_iteration=4, train_batches=4,
                             batch_size=32, capacity=8192, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=2,
                             generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path), om=om, log=seen.append)
    torch.cuda.synchronize()
    print(hist)
    assert hist["il_stored"] > 0 and hist["il_loss"] is not None and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 3 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["native_refreshes"] == 3 and hist["native_forwards"] > 0 and hist["memory"] > 0
    files = {}
    for name in ("il_model.pth", "rl_model_3.pth"):
        files[name] = torch.load(str(tmp_path / name), map_location="cpu")
        ref = sg.module(net_shape).state_dict()
        assert list(files[name]) == list(ref) and all(files[name][k].shape == ref[k].shape for k in ref)
        sg.module(net_shape).load_state_dict(files[name], strict=True)
        assert files[name]["mlp1.0.weight"].shape == (150, 65) and all(bool(torch.isfinite(v).all()) for v in files[name].values())
    assert not all(torch.equal(files["il_model.pth"][k], start[k]) for k in start)
    assert not all(torch.equal(files["rl_model_3.pth"][k], files["il_model.pth"][k]) for k in start)
    assert not torch.equal(files["rl_model_3.pth"]["mlp1.0.weight"][:, 17:], start["mlp1.0.weight"][:, 17:])  # the map columns learn
    # the refreshed weights decide: a network that takes them through refresh_from gives other values than the start
    net = SarlValueNet(start, device=DEV)
    policy = DeviceSarlPolicy(net, space, GAMMA, om=om)
    before = policy.decide(env)[1].clone()
    assert net.refresh_from(tr) is True
    after = policy.decide(env)[1].clone()
    fresh = DeviceSarlPolicy(SarlValueNet(tr.state_dict(), device=DEV), space, GAMMA, om=om).decide(env)[1]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after) and torch.equal(after, fresh)
    assert v0.shape == after.shape
    env.close()
