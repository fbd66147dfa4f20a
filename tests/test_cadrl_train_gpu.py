"""Training CADRL on the device: the gradient kernel (ebc_cadrl_grad) against the host build of the same rule, byte for byte,
at every batch size around the chunk, every row count and both widths, with and without n_valid and mask and over the
edge batches; canaries around its outputs; its refusals; CadrlTrainer native against autograd; the deciding blocks after
refresh_native; and the training schedule end to end.  Cases and the bar: tests/cadrl_grad_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from cadrl_cases import TOL_FACTOR, golden_run, golden_state_dict
from cadrl_grad_cases import (BATCHES, NARROW_WIDTHS, ROWS, WIDTHS, edge_batch, host_grad, host_pack, plain_batch, random_state_dict,
                              same_bytes)
from helpers import batch_from_init, load, params_of
from ebcsim import _abi, _capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xB6

_nets = {}


def device_net(wi):
    """(widths, state_dict, packed image by the header's pack, CadrlNet on the device) of a seeded network, once."""
    if wi not in _nets:
        from ebcsim.cadrl_train import CadrlNet
        sd = random_state_dict(WIDTHS[wi])
        _nets[wi] = (WIDTHS[wi], sd, host_pack(sd), CadrlNet(sd, 0))
    return _nets[wi]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_grad(net, rows, target, nv, mask, scale):
    """(grad, loss_sum, count, value, min_row) of one ebc_cadrl_grad on host arrays, every output poisoned before."""
    B = rows.shape[0]
    grad = torch.full((net.packed_floats(),), -7.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -7.0, dtype=torch.float64, device=DEV), torch.full((), -7, dtype=torch.int64, device=DEV)
    value, min_row = torch.full((B,), -7.0, dtype=torch.float32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    net.grad(_dev(rows), _dev(target), grad, loss, count, scale, _dev(nv), _dev(mask), value, min_row)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), min_row.cpu().numpy()


def assert_same(got, want, tag):
    assert same_bytes(got[0], want[0]), (tag, "grad", np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (tag, "loss_sum", got[1], want[1])
    assert got[2] == want[2], (tag, "count", got[2], want[2])
    assert same_bytes(got[3], want[3]), (tag, "value", got[3], want[3])
    assert same_bytes(got[4], want[4]), (tag, "min_row", got[4], want[4])


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("wi", range(len(WIDTHS)))
def test_kernel_equals_host_build_bytes(wi, R):
    """B in 1, 15, 16, 17, 33 at this width and row count: grad, loss_sum, count, value and min_row are the host build's,
    byte for byte, on plain batches without n_valid and mask and on the edge batches with both; the packed image on the
    device is the header's; a second call on the same inputs gives the same bytes."""
    widths, sd, P, net = device_net(wi)
    image = torch.empty(net.packed_floats(), dtype=torch.float32, device=DEV)
    assert same_bytes(net.get_packed(image).cpu().numpy(), P)
    for B in BATCHES:
        rows, target = plain_batch(widths, B, R)
        assert_same(kernel_grad(net, rows, target, None, None, 2.0 / B), host_grad(P, widths, rows, target, None, None, 2.0 / B), ("plain", B, R))
        rows, target, nv, mask, kinds = edge_batch(widths, B, R)
        want = host_grad(P, widths, rows, target, nv, mask, 2.0 / B)
        got = kernel_grad(net, rows, target, nv, mask, 2.0 / B)
        assert_same(got, want, ("edge", B, R, kinds))
        assert_same(kernel_grad(net, rows, target, nv, mask, 2.0 / B), got, ("again", B, R))
        assert_same(kernel_grad(net, rows, target, nv, None, 2.0 / B), host_grad(P, widths, rows, target, nv, None, 2.0 / B), ("no mask", B, R))


def test_a_nan_in_a_live_row_and_a_batch_without_live_states():
    widths, sd, P, net = device_net(1)
    rows, target = plain_batch(widths, 19, 2, seed=81)
    rows[17, 1, 3] = np.nan
    want = host_grad(P, widths, rows, target, None, None, 0.1)
    assert np.isnan(want[1]) and np.isnan(want[0]).any()
    assert_same(kernel_grad(net, rows, target, None, None, 0.1), want, "nan")
    mask = np.zeros(19, dtype=np.uint8)
    got = kernel_grad(net, rows, target, None, mask, 0.1)
    assert_same(got, host_grad(P, widths, rows, target, None, mask, 0.1), "dead")
    assert got[2] == 0 and got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()
    got = kernel_grad(net, rows[:0], target[:0], None, None, 0.1)
    assert got[2] == 0 and got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()


def test_more_chunks_than_one_launch_takes():
    """16 * 1024 + 21 states, one row each, the narrow network: the partials of 1026 chunks go through the float64 sums in
    two launches; the bytes are the host build's."""
    widths, sd, P, net = device_net(1)
    B = 16 * 1024 + 21
    rows, target = plain_batch(widths, B, 1, seed=82)
    mask = (np.arange(B) % 7 != 3).astype(np.uint8)
    assert_same(kernel_grad(net, rows, target, None, mask, 2.0 / B), host_grad(P, widths, rows, target, None, mask, 2.0 / B), "two launches")


def test_widest_network_and_most_rows():
    """The limits themselves: rows 64 wide, three layers of 256 units, 128 rows per state (115 KB of LDS, above what a launch
    gets by default), 5 states with ragged row counts: the host build's bytes."""
    from ebcsim.cadrl_train import CadrlNet
    widths = [64, 256, 256, 256, 1]
    sd = random_state_dict(widths)
    net, P = CadrlNet(sd, 0), host_pack(sd)
    rows, target = plain_batch(widths, 5, 128, seed=85)
    nv = np.array([128, 1, 77, 0, 200], dtype=np.int64)
    assert_same(kernel_grad(net, rows, target, nv, None, 0.4), host_grad(P, widths, rows, target, nv, None, 0.4), "widest")


def test_guard_words_around_the_outputs():
    """grad, value and min_row as slices of larger tensors filled with a canary: B = 17, R = 18, the bytes on both sides are
    intact and the insides are the host build's."""
    widths, sd, P, net = device_net(0)
    B, R, PF, pad = 17, 18, net.packed_floats(), 4096
    rows, target, nv, mask, _ = edge_batch(widths, B, R)
    raw = {k: torch.full((2 * pad + n * 4,), CANARY, dtype=torch.uint8, device=DEV) for k, n in (("grad", PF), ("value", B), ("min_row", B))}
    inside = {k: v[pad:v.numel() - pad] for k, v in raw.items()}
    grad, value, min_row = inside["grad"].view(torch.float32), inside["value"].view(torch.float32), inside["min_row"].view(torch.int32)
    loss, count = torch.zeros((), dtype=torch.float64, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    net.grad(_dev(rows), _dev(target), grad, loss, count, 2.0 / B, _dev(nv), _dev(mask), value, min_row)
    torch.cuda.synchronize()
    for k, v in raw.items():
        b = v.cpu().numpy()
        assert (b[:pad] == CANARY).all() and (b[-pad:] == CANARY).all(), k
    assert_same((grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), min_row.cpu().numpy()),
                host_grad(P, widths, rows, target, nv, mask, 2.0 / B), "guarded")


def _create(widths, n_layers=4):
    w = _abi.EbcCadrlNetWeights()
    w.struct_size = C.sizeof(w)
    w.n_layers = n_layers
    keep = []
    for i, v in enumerate(widths):
        w.widths[i] = v
    for l in range(4):
        keep.append((np.zeros((max(widths[l + 1], 1), max(widths[l], 1)), dtype=np.float32), np.zeros((max(widths[l + 1], 1),), dtype=np.float32)))
        w.weight[l], w.bias[l] = keep[-1][0].ctypes.data, keep[-1][1].ctypes.data
    h = C.c_void_p()
    rc = _capi.lib().ebc_cadrl_net_create(C.addressof(w), 0, C.byref(h))
    return rc, h, _capi.lib().ebc_last_error()


def test_refusals_and_capture():
    """Widths outside the limits, R > 128 and a capturing stream: EBC_ERR_UNSUPPORTED with a message that names the limit,
    nothing written, and the entry stays usable."""
    lib = _capi.lib()
    for widths, word in (([65, 150, 100, 100, 1], b"1 .. 64"), ([13, 257, 100, 100, 1], b"1 .. 256"), ([13, 150, 100, 300, 1], b"1 .. 256"),
                         ([13, 150, 0, 100, 1], b"1 .. 256"), ([13, 150, 100, 100, 2], b"exactly 1")):
        rc, h, msg = _create(widths)
        assert rc == _abi.ERR_UNSUPPORTED and word in msg and not h.value, (widths, msg)
    rc, h, msg = _create([13, 150, 100, 100, 1], n_layers=3)
    assert rc == _abi.ERR_UNSUPPORTED and b"exactly 4" in msg
    rc, h, msg = _create([64, 256, 256, 256, 1])  # the limits themselves are taken
    assert rc == _abi.OK and h.value
    assert lib.ebc_cadrl_net_destroy(h) == _abi.OK

    widths, sd, P, net = device_net(1)
    rows, target = plain_batch(widths, 3, 2, seed=83)
    want = host_grad(P, widths, rows, target, None, None, 1.0)
    grad = torch.full((net.packed_floats(),), -5.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -5.0, dtype=torch.float64, device=DEV), torch.full((), -5, dtype=torch.int64, device=DEV)
    big = torch.zeros((1, 129, widths[0]), dtype=torch.float32, device=DEV)
    with pytest.raises(_capi.EbcError) as err:
        net.grad(big, torch.zeros(1, device=DEV), grad, loss, count, 1.0)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "R > 128" in str(err.value)
    with pytest.raises(_capi.EbcError) as err:
        net.grad(torch.zeros((1, 2, widths[0] + 1), device=DEV), torch.zeros(1, device=DEV), grad, loss, count, 1.0)
    assert err.value.code == _abi.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5
    rd, td = _dev(rows), _dev(target)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        net.grad(rd, td, grad, loss, count, 1.0)  # scratch and the kernel's attributes are set before the capture
        side.synchronize()
        grad.fill_(-5.0)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError) as err:
                net.grad(rd, td, grad, loss, count, 1.0)
            with pytest.raises(_capi.EbcError) as err2:
                net.set_packed(grad)
            with pytest.raises(_capi.EbcError) as err3:
                net.get_packed(grad)
        finally:
            graph.capture_end()
        assert err.value.code == _abi.ERR_UNSUPPORTED and "captured" in str(err.value)
        assert err2.value.code == err3.value.code == _abi.ERR_UNSUPPORTED
        side.synchronize()
        assert bool((grad == -5.0).all())
        net.grad(rd, td, grad, loss, count, 1.0)
        side.synchronize()
    assert same_bytes(grad.cpu().numpy(), want[0]) and float(loss) == want[1] and int(count) == want[2]


def _float64_steps(z, sd, steps):
    """`steps` SGD steps over the golden's batches (cycled) with plain torch in float64 and float32: per step the loss
    and the weights of both."""
    from ebcsim.cadrl import CadrlModule
    out = {}
    for dtype in (torch.float64, torch.float32):
        m = CadrlModule.from_state_dict(sd).to(dtype)
        opt = torch.optim.SGD(m.parameters(), lr=float(z["lr"]), momentum=0.9)
        losses, weights = [], []
        for i in range(steps):
            a, b = z["batches"][i % len(z["batches"])]
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(m.value_network(torch.from_numpy(z["states"][a:b]).to(dtype)),
                                                torch.from_numpy(z["values"][a:b]).to(dtype)[:, None])
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            weights.append({k: v.detach().double().numpy().copy() for k, v in m.state_dict().items()})
        out[dtype] = (losses, weights)
    return out


def test_native_trainer_against_autograd_trainer():
    """Ten SGD steps of CadrlTrainer(native=True) and CadrlTrainer(native=False) on the device from the golden's start on the
    golden's batches: both stay, in every step's loss and every tensor, within TOL_FACTOR times torch's own float32 error
    against the same steps in float64 (CPU, measured here) of those float64 steps."""
    from ebcsim.cadrl_train import CadrlTrainer
    z = load("cadrl_one_trainer_steps")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0_")}
    steps = 10
    ref = _float64_steps(z, sd, steps)
    (l64, w64), (l32, w32) = ref[torch.float64], ref[torch.float32]
    trainers = {"native": CadrlTrainer(sd, device=DEV, optimizer="sgd", lr=float(z["lr"]), native=True),
                "autograd": CadrlTrainer(sd, device=DEV, optimizer="sgd", lr=float(z["lr"]), native=False)}
    assert trainers["native"].native and trainers["native"].net is not None and not trainers["autograd"].native
    states, values = torch.from_numpy(z["states"]).to(DEV), torch.from_numpy(z["values"]).to(DEV)
    for i in range(steps):
        a, b = z["batches"][i % len(z["batches"])]
        for name, tr in trainers.items():
            loss, count = tr.loss_and_grad(states[a:b, None, :], values[a:b], grad_scale=2.0 / (b - a))
            tr.step()
            mse, e_loss = float(loss) / int(count), abs(l32[i] - l64[i])
            got = tr.state_dict()
            worst = max(float(np.abs(got[k].numpy().astype(np.float64) - w64[i][k]).max()) / float(np.abs(w32[i][k] - w64[i][k]).max()) for k in sd)
            print("step %d %-8s loss %.9g (float64 %.9g, torch32 error %.3e), weights at most %.2f x torch32's error" % (
                i, name, mse, l64[i], e_loss, worst))
            assert int(count) == b - a and e_loss > 0 and abs(mse - l64[i]) <= TOL_FACTOR * e_loss, (i, name)
            assert worst <= TOL_FACTOR, (i, name, worst)
    assert l64[-1] < l64[0] and np.isfinite(l64).all()


def test_refresh_native_gives_the_decisions_of_a_fresh_network():
    """Three optimizer steps, then set_packed (inside step) and refresh_native: DeviceCadrlPolicy.decide on 5 envs of cadrl_a5
    gives the bytes (actions, values, choice) of a fresh CadrlValueNet built from trainer.state_dict()."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.cadrl import CadrlValueNet, DeviceCadrlPolicy
    from ebcsim.cadrl_train import CadrlTrainer
    z, meta, _, _ = golden_run("cadrl_a5")
    sd = golden_state_dict(meta)
    E = 5
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params_of(z), E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = CadrlValueNet(sd, device=DEV)
    policy = DeviceCadrlPolicy(net, z["action_space"], meta["gamma"])
    a0, v0 = policy.decide(env)
    tr = CadrlTrainer(sd, device=DEV, optimizer="sgd", lr=0.05)
    rows, target = plain_batch([13], 40, 3, seed=84)
    for _ in range(3):
        tr.loss_and_grad(_dev(rows), _dev(target), grad_scale=2.0 / 40)
        tr.step()
    image = torch.empty(tr.net.packed_floats(), dtype=torch.float32, device=DEV)
    assert torch.equal(tr.net.get_packed(image), tr.flat.detach())  # step() handed the kernel's object the new weights
    assert net.refresh_native(tr) is True and net.native_refreshes == 1
    a1, v1 = policy.decide(env)
    c1 = net.last_choice.clone()
    fresh = CadrlValueNet(tr.state_dict(), device=DEV)
    a2, v2 = DeviceCadrlPolicy(fresh, z["action_space"], meta["gamma"]).decide(env)
    torch.cuda.synchronize()
    assert same_bytes(v1.cpu().numpy(), v2.cpu().numpy()) and same_bytes(a1.cpu().numpy(), a2.cpu().numpy())
    assert torch.equal(c1, fresh.last_choice)
    assert not same_bytes(v1.cpu().numpy(), v0.cpu().numpy())  # the steps moved the values
    assert all(torch.equal(p.cpu(), tr.state_dict()[k]) for k, p in net.module.state_dict().items())
    assert net.refresh_native(tr.state_dict()) is True  # a state_dict of host tensors is taken too
    a3, v3 = policy.decide(env)
    assert same_bytes(v3.cpu().numpy(), v2.cpu().numpy())
    env.close()


def test_training_schedule_end_to_end(tmp_path):
    """run_cadrl_training on 8 envs of the one-human scene of cadrl_one: 40 imitation-learning steps with one epoch, then 2
    RL rounds of 3 decisions and 4 optimizer steps: finite losses, the blocks re-packed every round, and the saved files
    round-trip through CadrlModule.from_state_dict."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.cadrl import CadrlModule
    from ebcsim.cadrl_train import CadrlTrainer, run_cadrl_training
    z, meta, _, _ = golden_run("cadrl_one")
    E = 8
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params_of(z), E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    assert env.R == 1 and env.T == 13
    tr = CadrlTrainer(golden_state_dict(meta), device=DEV, optimizer="sgd", lr=0.01)
    hist = run_cadrl_training(env, tr, z["action_space"], meta["gamma"], il_steps=40, il_epochs=1, train_iterations=2,
                              steps_per_iteration=3, train_batches=4, batch_size=16, capacity=4096, target_update_interval=1,
                              generator=torch.Generator(device=DEV).manual_seed(3), output_dir=str(tmp_path), checkpoint_interval=1)
    torch.cuda.synchronize()
    print(hist)
    assert hist["il_stored"] > 0 and hist["il_loss"] is not None and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 2 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["native_refreshes"] == 2 and hist["native_forwards"] > 0
    for name in ("il_model.pth", "rl_model_1.pth", "rl_model_2.pth"):
        sd = torch.load(str(tmp_path / name), map_location="cpu")
        m = CadrlModule.from_state_dict(sd)
        assert [int(p.shape[0]) for k, p in m.state_dict().items() if k.endswith(".weight")] == [150, 100, 100, 1]
        assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    last = torch.load(str(tmp_path / "rl_model_2.pth"), map_location="cpu")
    assert all(torch.equal(last[k], v) for k, v in tr.state_dict().items())
    env.close()


def _generated_env(E, **overrides):
    """E envs of the one-human config on device-generated train scenes with a restart pool, as tools/train_cadrl.py builds them."""
    import configparser
    import os
    from cadrl_grad_cases import ROOT
    from ebcsim import actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "cadrl_one_human.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_plain.config"))
    params = ebc_config.params_from_config(cfg, pol, policy="cadrl")
    for k, v in overrides.items():
        setattr(params, k, v)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "train")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    env.generate_reset(gen, ebc_scene.COUNTER_OFFSET["train"])
    env.generate_pool(gen, ebc_scene.COUNTER_OFFSET["train"] + E, 8 * E)
    return env, ebc_actions.build_action_space(sc.robot.v_pref)


def test_training_schedule_on_generated_scenes_with_a_pool(tmp_path):
    """What tools/train_cadrl.py runs, small: 64 envs of the one-human config on generated scenes with a restart pool, 60
    imitation steps, then 6 RL rounds of 8 epsilon-greedy decisions (epsilon 0.5: random actions collide, and a collision's
    reward is the config's penalty) with an evaluation-sized second env opened and closed between the stages: every
    reward, target and loss is finite, episodes of the RL rounds reach the replay memory, the weights stay finite."""
    from ebcsim.cadrl import CadrlModule
    from ebcsim.cadrl_train import CadrlTrainer, run_cadrl_training
    env, space = _generated_env(64)
    assert all(np.isfinite(float(v)) for v in env.params.collision_penalty)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        tr = CadrlTrainer(CadrlModule(env.T, [150, 100, 100, 1]), device=DEV, optimizer="sgd", lr=0.01)
    seen = {}

    def after_il(h):
        other, _ = _generated_env(16)
        other.close()
        seen["il"] = dict(h)

    hist = run_cadrl_training(env, tr, space, 0.9, il_steps=60, il_epochs=1, train_iterations=6, steps_per_iteration=8, train_batches=4,
                              batch_size=32, capacity=8192, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=2,
                              generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path), after_il=after_il)
    torch.cuda.synchronize()
    print(hist)
    assert seen["il"]["il_stored"] > 0 and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 6 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["memory"] > hist["il_stored"]  # RL episodes ended and were stored
    assert all(bool(torch.isfinite(v).all()) for v in tr.state_dict().values())
    assert all(bool(torch.isfinite(v).all()) for v in torch.load(str(tmp_path / "rl_model_6.pth"), map_location="cpu").values())
    env.close()


def test_training_stops_at_the_first_value_that_is_not_finite(tmp_path):
    """An env whose success reward is NaN: the imitation stage's targets are NaN, run_cadrl_training raises before an
    optimizer step has seen them, the weights are the starting ones and no file is written."""
    from ebcsim.cadrl import CadrlModule
    from ebcsim.cadrl_train import CadrlTrainer, run_cadrl_training
    env, space = _generated_env(32, success_reward=float("nan"))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        tr = CadrlTrainer(CadrlModule(env.T, [150, 100, 100, 1]), device=DEV, optimizer="sgd", lr=0.01)
    start = tr.state_dict()
    with pytest.raises(FloatingPointError) as err:
        run_cadrl_training(env, tr, space, 0.9, il_steps=60, il_epochs=1, train_iterations=1, output_dir=str(tmp_path))
    assert "value target" in str(err.value)
    assert all(torch.equal(v, start[k]) for k, v in tr.state_dict().items()) and not list(tmp_path.iterdir())
    env.close()
