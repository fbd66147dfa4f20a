"""Training SAIL on the device: the gradient kernel (ebc_sail_grad) against the host build of the same rule, raw bytes of
grad, loss_sum, count and action, at the shapes where it can go wrong; its isolation and determinism; ebc_sail_set_packed
and _get_packed; and demonstrations -> fit -> a saved file that decides.  Cases: tests/sail_grad_cases.py."""
import configparser
import ctypes as C

import numpy as np
import pytest
import torch

from sail_cases import golden, host_forward, random_state_dict, same_bytes
from sail_grad_cases import chunk, group, host_grad, host_pack, masked_batch, plain_batch
from ebcsim import _abi, _capi
from helpers import Guarded, params_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADULTS = [2, 5, 9, 32]
_nets = {}


def net_of(N, scale=8):
    from ebcsim.sail import SailNet
    if (N, scale) not in _nets:
        _nets[N, scale] = SailNet(random_state_dict(N, scale), device=DEV)
    return _nets[N, scale]


def env_counts(N):
    G, Cn = group(N), chunk()
    return sorted({E for E in (1, G - 1, G + 1, Cn - 1, Cn, Cn + 1, 2 * Cn + 3) if E >= 1})


def grad_call(handle, robot, ob, target, n_rows, mask, grad_scale, grad_ptr, loss, count, action_ptr, E=None, R=None, check=True):
    """One ebc_sail_grad on the current stream; robot, ob, target, n_rows, mask are device tensors (or None)."""
    a = _abi.EbcSailGradArgs()
    a.struct_size = C.sizeof(a)
    a.E, a.R = int(ob.shape[0] if E is None else E), int(ob.shape[1] if R is None else R)
    a.grad_scale = float(grad_scale)
    a.robot, a.ob, a.target = robot.data_ptr(), ob.data_ptr(), target.data_ptr()
    a.n_rows = None if n_rows is None else n_rows.data_ptr()
    a.sample_mask = None if mask is None else mask.data_ptr()
    a.grad, a.loss_sum, a.count, a.action = grad_ptr, loss.data_ptr(), count.data_ptr(), action_ptr
    rc = _capi.lib().ebc_sail_grad(handle, torch.cuda.current_stream().cuda_stream, C.addressof(a))
    if check:
        _capi.check(rc)
    return rc


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_grad(net, robot, ob, target, n_rows=None, mask=None, grad_scale=1.0, want_action=True):
    """(grad, loss_sum, count, action) of the kernel on host arrays: grad and action between canaries, every element written."""
    E, PF = ob.shape[0], int(host_pack_len(net.adult_num))
    gg = Guarded((PF,), torch.float32, device=DEV)
    ga = Guarded((E, 2), torch.float64, device=DEV) if want_action else None
    loss = torch.full((3,), -5.0, dtype=torch.float64, device=DEV)
    count = torch.full((3,), -5, dtype=torch.int64, device=DEV)
    grad_call(net.native()._h, to_dev(robot), to_dev(ob), to_dev(target), to_dev(n_rows), to_dev(mask), grad_scale, gg.ptr, loss[1:], count[1:],
              ga.ptr if want_action else None)
    torch.cuda.synchronize()
    loss, count = loss.cpu().numpy(), count.cpu().numpy()
    assert loss[0] == loss[2] == -5.0 and count[0] == count[2] == -5  # the neighbours of the two scalars
    return gg.check(), float(loss[1]), int(count[1]), ga.check() if want_action else None


def host_pack_len(N):
    from ebcsim.sail_train import packed_floats
    n = C.c_int64(0)
    _capi.check(_capi.lib().ebc_sail_packed_floats(net_of(N).native()._h, C.byref(n)))
    assert n.value == packed_floats(N)
    return n.value


def assert_same(tag, got, want):
    g, l, c, a = got
    wg, wl, wc, wa = want
    assert same_bytes(g, wg), (tag, "grad", np.argwhere(g.view(np.int32) != wg.view(np.int32))[:4].ravel().tolist())
    assert np.float64(l).tobytes() == np.float64(wl).tobytes(), (tag, "loss", l, wl)
    assert c == wc, (tag, "count", c, wc)
    if a is not None:
        assert same_bytes(a, wa), (tag, "action", np.argwhere(a.view(np.int64) != wa.view(np.int64))[:4].tolist())


@pytest.mark.parametrize("N", ADULTS)
def test_kernel_equals_host_build_bytes(N):
    """Every env count of this adult_num (1, G - 1, G + 1, C - 1, C, C + 1, 2 C + 3: a partial group, a partial chunk, one
    env per group at 32 adults), R = N and R = N + 3 with NaN and infinities past N, plain batches and batches with row
    counts other than N, arrived envs and a sample mask all at once (those envs full of NaN): grad, loss_sum, count and
    action have the host build's bytes; action is ebc_sail_forward's."""
    net, sd = net_of(N), random_state_dict(N, 8)
    P = host_pack(sd)
    for R in (N, N + 3):
        for E in env_counts(N):
            robot, ob, target = plain_batch(N, E, R, None)
            want = host_grad(P, N, robot, ob, target, grad_scale=1.0 / E)
            assert_same("plain N %d E %d R %d" % (N, E, R), kernel_grad(net, robot, ob, target, grad_scale=1.0 / E), want)
            assert want[2] == E and np.isfinite(want[0]).all()
            robot, ob, target, n_rows, mask, live = masked_batch(N, E, R, 50 + E, poison=True)
            scale = 1.0 / max(int(live.sum()), 1)
            want = host_grad(P, N, robot, ob, target, n_rows, mask, scale)
            assert_same("masked N %d E %d R %d" % (N, E, R), kernel_grad(net, robot, ob, target, n_rows, mask, scale), want)
            assert want[2] == int(live.sum()) and np.isfinite(want[0]).all()
            assert same_bytes(want[3], host_forward(sd, robot, ob, n_rows)[0])


@pytest.mark.parametrize("which", ["n_rows", "arrived", "sample_mask"])
def test_each_kind_of_masking_alone(which):
    N, R = 5, 8
    E = 2 * chunk() + 3
    net, P = net_of(N), host_pack(random_state_dict(N, 8))
    robot, ob, target = plain_batch(N, E, R, 61)
    n_rows = mask = None
    if which == "n_rows":
        n_rows = np.where(np.arange(E) % 3 == 1, N + 1, N).astype(np.int64)
    elif which == "arrived":
        robot[::3, 5], robot[::3, 6] = robot[::3, 0] + 0.1, robot[::3, 1] - 0.1
    else:
        mask = (np.arange(E) % 3 != 2).astype(np.uint8)
    want = host_grad(P, N, robot, ob, target, n_rows, mask, 0.25)
    assert 0 < want[2] < E
    assert_same(which, kernel_grad(net, robot, ob, target, n_rows, mask, 0.25), want)
    assert_same(which + " no action", kernel_grad(net, robot, ob, target, n_rows, mask, 0.25, want_action=False), want)


def test_two_launches_give_the_same_bytes_and_empty_batches_give_zeros():
    N = 5
    E = 2 * chunk() + 3
    net = net_of(N)
    robot, ob, target, n_rows, mask, live = masked_batch(N, E, N + 3, 62, poison=True)
    first = kernel_grad(net, robot, ob, target, n_rows, mask, 0.5)
    second = kernel_grad(net, robot, ob, target, n_rows, mask, 0.5)
    assert_same("repeat", second, first)
    g, loss, count, _ = kernel_grad(net, robot, ob, target, n_rows, np.zeros(E, np.uint8), 0.5)
    assert (g.view(np.int32) == 0).all() and loss == 0.0 and count == 0
    g, loss, count, _ = kernel_grad(net, robot[:0], ob[:0], target[:0], None, None, 0.5, want_action=False)
    assert (g.view(np.int32) == 0).all() and loss == 0.0 and count == 0


def test_refusals_and_capture():
    """R < adult_num is refused before anything is launched; a stream under capture is refused with EBC_ERR_UNSUPPORTED and
    the stream stays usable."""
    lib = _capi.lib()
    N, E = 5, 9
    net, P = net_of(N), host_pack(random_state_dict(N, 8))
    robot, ob, target = plain_batch(N, E, N + 3, 63)
    want = host_grad(P, N, robot, ob, target, grad_scale=0.5)
    rd, od, td = to_dev(robot), to_dev(ob), to_dev(target)
    grad = torch.full((len(P),), -5.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((1,), -5.0, dtype=torch.float64, device=DEV), torch.full((1,), -5, dtype=torch.int64, device=DEV)
    h = net.native()._h
    assert grad_call(h, rd, od, td, None, None, 0.5, grad.data_ptr(), loss, count, None, R=N - 1, check=False) == _abi.ERR_INVALID
    assert b"R < adult_num" in lib.ebc_last_error()
    torch.cuda.synchronize()
    assert (grad == -5.0).all() and float(loss) == -5.0 and int(count) == -5
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        grad_call(h, rd, od, td, None, None, 0.5, grad.data_ptr(), loss, count, None)  # scratch and the LDS limit are set up outside
        side.synchronize()
        graph.capture_begin()
        try:
            rc = grad_call(h, rd, od, td, None, None, 0.5, grad.data_ptr(), loss, count, None, check=False)
            rc_set = lib.ebc_sail_set_packed(h, torch.cuda.current_stream().cuda_stream, grad.data_ptr())
        finally:
            graph.capture_end()
        assert rc == _abi.ERR_UNSUPPORTED and rc_set == _abi.ERR_UNSUPPORTED and b"captured" in lib.ebc_last_error()
        grad.fill_(-5.0)
        grad_call(h, rd, od, td, None, None, 0.5, grad.data_ptr(), loss, count, None)
        side.synchronize()
    assert same_bytes(grad.cpu().numpy(), want[0]) and float(loss) == want[1] and int(count) == want[2]


def test_set_packed_and_get_packed():
    """After ebc_sail_set_packed a forward has the bytes of a fresh handle made from the same weights; get_packed returns
    what was set; an env the network is attached to rolls out with the new weights."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailNet
    from ebcsim.sail_train import pack_state_dict
    from sail_rollout_cases import golden_batch
    lib = _capi.lib()
    N = 5
    old, new = random_state_dict(N, 1), random_state_dict(N, 8)
    net, fresh = SailNet(old, device=DEV), SailNet(new, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    robot, ob, target = plain_batch(N, 11, N + 2, 64)
    rd, od = to_dev(robot), to_dev(ob)
    before = net.forward(rd, od)[0].cpu().numpy()
    image = pack_state_dict(new).to(DEV)
    got = Guarded((image.numel(),), torch.float32, device=DEV)
    _capi.check(lib.ebc_sail_get_packed(net.native()._h, stream, got.ptr))
    torch.cuda.synchronize()
    assert same_bytes(got.check(), host_pack(old))
    _capi.check(lib.ebc_sail_set_packed(net.native()._h, stream, image.data_ptr()))
    after, feat = net.forward(rd, od)
    want, want_feat = fresh.forward(rd, od)
    assert same_bytes(after.cpu().numpy(), want.cpu().numpy()) and same_bytes(feat.cpu().numpy(), want_feat.cpu().numpy())
    assert not same_bytes(after.cpu().numpy(), before)
    assert same_bytes(after.cpu().numpy(), host_forward(new, robot, ob)[0])
    got = Guarded((image.numel(),), torch.float32, device=DEV)
    _capi.check(lib.ebc_sail_get_packed(net.native()._h, stream, got.ptr))
    torch.cuda.synchronize()
    assert same_bytes(got.check(), image.cpu().numpy())
    # an attached env: one step with the old weights, then set_packed, then three steps: those of a handle created from
    # the new weights, and not those of the old weights
    params, batch = golden_batch(4)
    old_image = pack_state_dict(old).to(DEV)

    def three_steps(policy, first=None):
        env = BatchedEnv(params, 4, batch.N, batch.S)
        env.reset(batch)
        env.use_torch_stream()
        if first is not None:
            first(env)
            env.reset(batch)
        outs = env.alloc_step_k_outputs(3, ("robot_action_out", "reward"))
        policy.rollout(env, 3, outs)
        torch.cuda.synchronize()
        env.close()
        return outs["robot_action_out"].cpu().numpy()

    want_new = three_steps(DeviceSailPolicy(fresh))
    _capi.check(lib.ebc_sail_set_packed(net.native()._h, stream, old_image.data_ptr()))
    pol = DeviceSailPolicy(net)
    got_old = three_steps(pol)

    def attach_then_set(env):
        pol.rollout(env, 1, env.alloc_step_k_outputs(1, ("robot_action_out", "reward")))  # attached, used with the old weights
        _capi.check(lib.ebc_sail_set_packed(net.native()._h, stream, image.data_ptr()))

    got_new = three_steps(pol, attach_then_set)
    assert np.isfinite(got_old).all() and same_bytes(got_new, want_new) and not same_bytes(got_old, got_new)


def a5_env(E, seed):
    """E envs of the A5 config of the SAIL goldens on device-generated scenes, with a pool for the restarts."""
    from ebcsim import scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    z, meta = golden("sail_a5")[:2]
    cfg = configparser.RawConfigParser()
    cfg.read_string(meta["config_text"])
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "train")
    env = BatchedEnv(params_of(z), E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    env.generate_reset(gen, seed)
    env.generate_pool(gen, seed + E, 2 * E)
    return env


def test_demonstrations_fit_and_decide(tmp_path):
    """32 envs x 64 steps of the ORCA robot on the A5 config with device scenes, then 3 epochs: episodes ended in ReachGoal
    inside the window (a condition on the inputs: the goal is 6 m away at 0.175 m per step, so no episode can end before
    step 35, and at 40 steps none had), the last epoch's loss is below the first's, and the saved file drives
    DeviceSailPolicy.decide to finite actions."""
    from ebcsim.sail import DeviceSailPolicy, SailNet
    from ebcsim.sail_train import SailTrainer, collect_sail_demos, fit
    env = a5_env(32, 2000)
    demos = collect_sail_demos(env, 64, safety_space=0.15)
    print("kept %d steps of %d episodes" % (demos["steps"], demos["episodes"]))
    assert demos["steps"] > 0 and demos["robot"].shape[0] == demos["steps"]
    assert bool((demos["n_rows"] == 5).all()) and bool(torch.isfinite(demos["target"]).all())
    tr = SailTrainer(golden("sail_a5")[2], device=DEV, optimizer="adam", lr=1e-3)
    assert tr.native is True
    losses = fit(tr, demos, epochs=3, batch_size=64, generator=torch.Generator(device=DEV).manual_seed(7))
    print("losses", losses)
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[-1] < losses[0]
    path = str(tmp_path / "sail_model.pth")
    tr.save(path)
    net = SailNet.load(path, device=DEV)
    actions, _ = DeviceSailPolicy(net).decide(env)
    mine, _ = DeviceSailPolicy(tr.net).decide(env)  # the trained handle itself: the same weights
    torch.cuda.synchronize()
    assert bool(torch.isfinite(actions).all()) and bool(actions.abs().sum() > 0) and torch.equal(actions, mine)
    env.close()


def test_native_gradient_is_close_to_autograd_on_the_device():
    """The trainer's two paths on the same batch: the kernel's gradient within 1e-4 of the largest entry of torch
    autograd's (both float32 evaluations of the same sums; the host build's bound is in test_sail_train_cpu.py)."""
    from ebcsim.sail_train import SailTrainer
    N, E = 5, 70
    sd = random_state_dict(N, 8)
    robot, ob, target, n_rows, mask, live = masked_batch(N, E, N + 1, 65, poison=True)
    args = [to_dev(a) for a in (robot, ob, target, n_rows, mask)]
    a, b = SailTrainer(sd, device=DEV, native=True), SailTrainer(sd, device=DEV, native=False)
    la, ca = a.loss_and_grad(*args)
    lb, cb = b.loss_and_grad(*args)
    assert int(ca) == int(cb) == int(live.sum()) and abs(float(la) - float(lb)) <= 1e-5 * float(lb)
    ga, gb = a.flat.grad.cpu().numpy(), b.flat.grad.cpu().numpy()
    assert np.isfinite(ga).all() and np.abs(ga - gb).max() <= 1e-4 * np.abs(gb).max()
