"""Training LSTM-RL on the device: the gradient kernel (ebc_lstm_grad) against the host build of the same rule, byte for
byte, at every batch size around the chunk, every row count and both networks, with and without n_valid and mask and over
the edge batches; h_n against the scan that decides; the largest R the entry takes; more chunks than one launch takes;
canaries around its outputs; its refusals; LstmTrainer native against autograd; the deciding network after refresh_from;
and the training schedule end to end.  Cases and the bar: tests/lstm_grad_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from lstm_grad_cases import (BATCHES, NETS, REFERENCE_NET1, REFERENCE_NET2, ROOT, ROWS, TOL_FACTOR, chunk, edge_batch, golden_rows, host_grad,
                             host_pack, max_chunks, module, plain_batch, random_state_dict, same_bytes)
from helpers import batch_from_init, load, params_of
from ebcsim import _abi, _capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xB6

_nets = {}


def device_net(ni):
    """(net, state_dict, packed image by the header's pack, LstmNet on the device) of a seeded network, once."""
    if ni not in _nets:
        from ebcsim.lstm_train import LstmNet
        sd = random_state_dict(NETS[ni], scale=4.0 if ni >= 2 else 1.0)
        _nets[ni] = (NETS[ni], sd, host_pack(sd), LstmNet(sd, 0))
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
    assert same_bytes(got[0], want[0]), (tag, "grad", np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (tag, "loss_sum", got[1], want[1])
    assert got[2] == want[2], (tag, "count", got[2], want[2])
    assert same_bytes(got[3], want[3]), (tag, "value", got[3], want[3])
    assert same_bytes(got[4], want[4]), (tag, "joint", got[4], want[4])


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("ni", [2, 3], ids=["narrow_mlp1", "narrow_plain"])
def test_kernel_equals_host_build_bytes(ni, R):
    """B in 1, C - 1, C, C + 1, 2 C + 1 at the narrow widths and this row count: grad, loss_sum, count, value and joint are
    the host build's, byte for byte, on plain batches without n_valid and mask and on the edge batches (n_valid holding 0,
    1, R, R + 3 and -1, NaN in every padding row) with a mask and without; the packed image on the device is the header's; a
    second call on the same inputs gives the same bytes."""
    net, sd, P, dn = device_net(ni)
    image = torch.empty(dn.packed_floats(), dtype=torch.float32, device=DEV)
    assert same_bytes(dn.get_packed(image).cpu().numpy(), P)
    for B in BATCHES:
        rows, target = plain_batch(net, B, R)
        assert_same(kernel_grad(dn, rows, target, None, None, 2.0 / B), host_grad(P, net, rows, target, None, None, 2.0 / B), ("plain", B, R))
        rows, target, nv, mask, kinds = edge_batch(net, B, R)
        got = kernel_grad(dn, rows, target, nv, mask, 2.0 / B)
        assert_same(got, host_grad(P, net, rows, target, nv, mask, 2.0 / B), ("edge", B, R, kinds))
        assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), got, ("again", B, R))
        assert_same(kernel_grad(dn, rows, target, nv, None, 2.0 / B), host_grad(P, net, rows, target, nv, None, 2.0 / B), ("no mask", B, R))


@pytest.mark.parametrize("B,R", [(1, 1), (chunk() + 1, 5), (2 * chunk() + 1, 10)])
@pytest.mark.parametrize("ni", [0, 1], ids=["mlp1", "plain"])
def test_kernel_equals_host_build_bytes_at_the_reference_widths(ni, B, R):
    net, sd, P, dn = device_net(ni)
    rows, target = plain_batch(net, B, R)
    assert_same(kernel_grad(dn, rows, target, None, None, 2.0 / B), host_grad(P, net, rows, target, None, None, 2.0 / B), ("plain", B, R))
    rows, target, nv, mask, kinds = edge_batch(net, B, R)
    assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), host_grad(P, net, rows, target, nv, mask, 2.0 / B), ("edge", B, R, kinds))


@pytest.mark.parametrize("ni", [1, 3], ids=["reference", "narrow"])
def test_h_n_is_the_deciding_scans(ni):
    """ValueNetwork1: joint[:, S:] is ebc_lstm_forward's h_n on the same rows and lengths, bit for bit (n_valid 0 leaves 0 in
    both), and joint[:, :S] is row 0's self state."""
    from ebcsim.lstm_rl import _NativeLstm
    net, sd, P, dn = device_net(ni)
    S, B, R = net[1], 2 * chunk() + 1, 5
    rows, target, nv, mask, kinds = edge_batch(net, B, R)
    got = kernel_grad(dn, rows, target, nv, None, 1.0)
    lstm = module(net).lstm
    lstm.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("lstm.")})
    scan = _NativeLstm(lstm, 0)
    x = _dev(rows)
    h = scan(x.view(B * R, net[0][0]), B, R, _dev(nv).clamp(0, R))
    torch.cuda.synchronize()
    assert same_bytes(got[4][:, S:], h.cpu().numpy()), kinds
    n = np.clip(nv, 0, R)
    assert same_bytes(got[4][n > 0, :S], rows[n > 0, 0, :S]) and (got[4][n == 0].view(np.uint32) == 0).all()


def test_a_nan_in_a_live_row_and_a_batch_without_live_states():
    net, sd, P, dn = device_net(2)
    rows, target = plain_batch(net, 7, 2, seed=81)
    rows[5, 1, 3] = np.nan
    want = host_grad(P, net, rows, target, None, None, 0.1)
    assert np.isnan(want[1]) and np.isnan(want[0]).any()
    assert_same(kernel_grad(dn, rows, target, None, None, 0.1), want, "nan")
    mask = np.zeros(7, dtype=np.uint8)
    got = kernel_grad(dn, rows, target, None, mask, 0.1)
    assert_same(got, host_grad(P, net, rows, target, None, mask, 0.1), "dead")
    assert got[2] == 0 and got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()
    got = kernel_grad(dn, rows[:0], target[:0], None, None, 0.1)
    assert got[2] == 0 and got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()


@pytest.mark.parametrize("ni", [0, 1], ids=["mlp1", "plain"])
def test_the_largest_r_runs_and_one_more_is_refused(ni):
    """ebc_lstm_net_grad_max_rows at the reference widths: at least 10, it runs and gives the host build's bytes; R + 1 is
    EBC_ERR_UNSUPPORTED and leaves every output untouched."""
    net, sd, P, dn = device_net(ni)
    R = dn.grad_max_rows()
    assert R >= 10
    B = chunk() + 1
    rows, target = plain_batch(net, B, R, seed=86)
    nv = np.array([R, 1, R + 3, R - 1, R][:B], dtype=np.int64)
    assert_same(kernel_grad(dn, rows, target, nv, None, 0.4), host_grad(P, net, rows, target, nv, None, 0.4), "largest R")
    grad = torch.full((dn.packed_floats(),), -5.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -5.0, dtype=torch.float64, device=DEV), torch.full((), -5, dtype=torch.int64, device=DEV)
    value, joint = torch.full((2,), -5.0, dtype=torch.float32, device=DEV), torch.full((2, dn.joint_dim), -5.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_capi.EbcError) as err:
        dn.grad(torch.zeros((2, R + 1, net[0][0]), dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV), grad, loss, count, 1.0,
                value=value, joint=joint)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "LDS" in str(err.value) and "R = %d" % (R + 1) in str(err.value)
    torch.cuda.synchronize()
    assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5 and bool((value == -5.0).all()) and bool((joint == -5.0).all())
    assert device_net(ni + 2)[3].grad_max_rows() > R  # the narrow network takes more rows: asked, not guessed


def test_more_chunks_than_one_launch_takes():
    """C * EBC_LSTM_GRAD_MAX_CHUNKS + 2 C + 1 states, two rows each, the narrow network with mlp1: the partials go through
    the float64 sums in two launches; the bytes are the host build's."""
    net, sd, P, dn = device_net(2)
    B = chunk() * max_chunks() + 2 * chunk() + 1
    rows, target = plain_batch(net, B, 2, seed=82)
    mask = (np.arange(B) % 7 != 3).astype(np.uint8)
    nv = (1 + np.arange(B) % 2).astype(np.int64)
    assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), host_grad(P, net, rows, target, nv, mask, 2.0 / B), "two launches")


def test_guard_words_around_the_outputs():
    """grad, value and joint as slices of larger tensors filled with a canary: B = 2 C + 1, R = 5, the bytes on both sides
    are intact and the insides are the host build's."""
    net, sd, P, dn = device_net(2)
    B, R, PF, pad = 2 * chunk() + 1, 5, dn.packed_floats(), 4096
    rows, target, nv, mask, _ = edge_batch(net, B, R)
    raw = {k: torch.full((2 * pad + n * 4,), CANARY, dtype=torch.uint8, device=DEV)
           for k, n in (("grad", PF), ("value", B), ("joint", B * dn.joint_dim), ("loss", 2), ("count", 2))}
    inside = {k: v[pad:v.numel() - pad] for k, v in raw.items()}
    grad, value, joint = inside["grad"].view(torch.float32), inside["value"].view(torch.float32), inside["joint"].view(torch.float32)
    loss, count = inside["loss"].view(torch.float64).reshape(()), inside["count"].view(torch.int64).reshape(())
    dn.grad(_dev(rows), _dev(target), grad, loss, count, 2.0 / B, _dev(nv), _dev(mask), value, joint)
    torch.cuda.synchronize()
    for k, v in raw.items():
        b = v.cpu().numpy()
        assert (b[:pad] == CANARY).all() and (b[-pad:] == CANARY).all(), k
    assert_same((grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), joint.cpu().numpy().reshape(B, dn.joint_dim)),
                host_grad(P, net, rows, target, nv, mask, 2.0 / B), "guarded")


def _create(T=13, mlp1=(150, 100, 100, 50), H=50, mlp=(150, 100, 100, 1), S=6, n_mlp1=None, n_mlp=4, lstm_in=None):
    """ebc_lstm_net_create on zero weights of the given shape -> (rc, handle, message)."""
    w = _abi.EbcLstmNetWeights()
    w.struct_size = C.sizeof(w)
    w.n_mlp1, w.n_mlp = (4 if mlp1 else 0) if n_mlp1 is None else n_mlp1, n_mlp
    w.self_state_dim, w.input_dim, w.hidden_dim = S, T, H
    w.lstm_input_dim = (mlp1[3] if mlp1 else T) if lstm_in is None else lstm_in
    keep = []
    for i, v in enumerate(list(mlp1 or (0, 0, 0, 0)) + list(mlp)):
        w.widths[i] = v
        keep.append((np.zeros((max(v, 1), 600), dtype=np.float32), np.zeros((max(v, 1),), dtype=np.float32)))
        w.weight[i], w.bias[i] = keep[-1][0].ctypes.data, keep[-1][1].ctypes.data
    cell = [np.zeros((4 * max(H, 1), 600), dtype=np.float32) for _ in range(4)]
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = (a.ctypes.data for a in cell)
    h = C.c_void_p()
    rc = _capi.lib().ebc_lstm_net_create(C.addressof(w), 0, C.byref(h))
    return rc, h, _capi.lib().ebc_last_error()


def test_refusals_and_capture():
    """Widths outside the limits, layer counts other than 0 or 4 / 4, a wrong T and a capturing stream:
    EBC_ERR_UNSUPPORTED (a wrong T: EBC_ERR_INVALID) with a message that names the limit, nothing written, and the entry
    stays usable.  The capture is begun and ended, never replayed."""
    lib = _capi.lib()
    for kw, word in ((dict(T=65), b"1 .. 64"), (dict(mlp1=(257, 100, 100, 50)), b"1 .. 256"), (dict(mlp1=(150, 100, 100, 65)), b"1 .. 64"),
                     (dict(mlp1=None, T=13, H=65), b"1 .. 64"), (dict(H=0), b"1 .. 64"), (dict(mlp=(150, 0, 100, 1)), b"1 .. 256"),
                     (dict(mlp=(300, 100, 100, 1)), b"1 .. 256"), (dict(mlp=(150, 100, 100, 2)), b"exactly 1"), (dict(S=14), b"self_state_dim"),
                     (dict(S=-1), b"self_state_dim"), (dict(n_mlp1=2), b"0 or 4 / 4"), (dict(n_mlp=3), b"0 or 4 / 4")):
        rc, h, msg = _create(**kw)
        assert rc == _abi.ERR_UNSUPPORTED and word in msg and not h.value, (kw, msg)
    rc, h, msg = _create(lstm_in=49)
    assert rc == _abi.ERR_INVALID and not h.value, msg
    for kw in (dict(T=64, mlp1=(256, 256, 256, 64), H=64, mlp=(256, 256, 256, 1), S=64), dict(T=64, mlp1=None, H=64, mlp=(256, 256, 256, 1), S=0)):
        rc, h, msg = _create(**kw)  # the limits themselves are taken
        assert rc == _abi.OK and h.value, (kw, msg)
        rows_out = C.c_int(-1)
        assert lib.ebc_lstm_net_grad_max_rows(h, C.byref(rows_out)) == _abi.OK and 1 <= rows_out.value < 26
        assert lib.ebc_lstm_net_destroy(h) == _abi.OK
    assert lib.ebc_lstm_grad(None, None, None) == _abi.ERR_INVALID

    net, sd, P, dn = device_net(2)
    rows, target = plain_batch(net, 3, 2, seed=83)
    want = host_grad(P, net, rows, target, None, None, 1.0)
    grad = torch.full((dn.packed_floats(),), -5.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -5.0, dtype=torch.float64, device=DEV), torch.full((), -5, dtype=torch.int64, device=DEV)
    with pytest.raises(_capi.EbcError) as err:
        dn.grad(torch.zeros((1, 2, net[0][0] + 1), device=DEV), torch.zeros(1, device=DEV), grad, loss, count, 1.0)
    assert err.value.code == _abi.ERR_INVALID and "wide" in str(err.value)
    a = _abi.EbcLstmGradArgs()
    a.struct_size = C.sizeof(a)
    a.B, a.R, a.T, a.grad_scale = 1, 2, net[0][0], 1.0
    assert lib.ebc_lstm_grad(dn._h, None, C.addressof(a)) == _abi.ERR_INVALID  # null grad, loss_sum, count
    torch.cuda.synchronize()
    assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5
    rd, td = _dev(rows), _dev(target)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dn.grad(rd, td, grad, loss, count, 1.0)  # scratch and the kernel's attributes are set before the capture
        side.synchronize()
        grad.fill_(-5.0)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError) as err:
                dn.grad(rd, td, grad, loss, count, 1.0)
            with pytest.raises(_capi.EbcError) as err2:
                dn.set_packed(grad)
            with pytest.raises(_capi.EbcError) as err3:
                dn.get_packed(grad)
        finally:
            graph.capture_end()
        assert err.value.code == _abi.ERR_UNSUPPORTED and "captured" in str(err.value)
        assert err2.value.code == err3.value.code == _abi.ERR_UNSUPPORTED
        side.synchronize()
        assert bool((grad == -5.0).all())
        dn.grad(rd, td, grad, loss, count, 1.0)
        side.synchronize()
    assert same_bytes(grad.cpu().numpy(), want[0]) and float(loss) == want[1] and int(count) == want[2]


# ---------------------------------------------------------------------------------------------- trainer and schedule
def _memory(two):
    """A small memory of golden rows: the five-adult run's states and recorded values, and a seeded reference-width network."""
    _, rows, values = golden_rows("lstm_interaction_a5" if two else "lstm_plain_a5")
    return random_state_dict(REFERENCE_NET2 if two else REFERENCE_NET1, seed=5), rows, values, 0.01


def _float64_steps(sd, states, values, lr, steps):
    """`steps` SGD steps on the whole memory with plain torch (LstmModule) in float64 on the CPU and in float32 on the CPU and
    on the device: per step the loss and the weights of each."""
    from ebcsim.lstm_train import module_of
    out = {}
    for key, dtype, device in (("f64", torch.float64, "cpu"), ("f32_cpu", torch.float32, "cpu"), ("f32_dev", torch.float32, DEV)):
        m = module_of(sd).to(dtype).to(device)
        opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9)
        x, y = torch.from_numpy(states).to(dtype).to(device), torch.from_numpy(values).to(dtype).to(device)
        losses, weights = [], []
        for i in range(steps):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(m(x).squeeze(1), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            weights.append({k: v.detach().double().cpu().numpy().copy() for k, v in m.state_dict().items()})
        out[key] = (losses, weights)
    return out


def _ratio(err, err_torch32):
    """err / err_torch32; a tensor torch's float32 steps leave exactly on the float64 ones has no yardstick and must be
    exact here too."""
    return err / err_torch32 if err_torch32 > 0 else (0.0 if err == 0 else float("inf"))


@pytest.mark.parametrize("two", [True, False], ids=["mlp1", "plain"])
def test_native_trainer_against_autograd_trainer(two):
    """Three SGD steps of LstmTrainer(native=True) and LstmTrainer(native=False) on the device from a seeded reference-width
    network on the 80 states of a golden run: both stay, in every step's loss and every tensor, within TOL_FACTOR times
    torch's own float32 error against the same steps in float64 (measured here) of those float64 steps.  The yardstick is
    that of test_sarl_train_gpu.test_native_trainer_against_autograd_trainer: the larger of torch's two float32 forms'
    errors (the CPU's and the device's), for the loss and for every tensor.  Neither looks at a trainer's result."""
    from ebcsim.lstm_train import LstmTrainer
    sd, states, values, lr = _memory(two)
    steps = 3
    ref = _float64_steps(sd, states, values, lr, steps)
    (l64, w64), (l32c, w32c), (l32d, w32d) = ref["f64"], ref["f32_cpu"], ref["f32_dev"]
    trainers = {"native": LstmTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=True),
                "autograd": LstmTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=False)}
    assert trainers["native"].native and trainers["native"].net is not None and not trainers["autograd"].native
    xs, ys = torch.from_numpy(states).to(DEV), torch.from_numpy(values).to(DEV)
    n = len(values)
    for i in range(steps):
        for name, tr in trainers.items():
            loss, count = tr.loss_and_grad(xs, ys, grad_scale=2.0 / n)
            tr.step()
            mse, e_loss = float(loss) / int(count), max(abs(l32c[i] - l64[i]), abs(l32d[i] - l64[i]))
            got = tr.state_dict()
            ratios = {k: _ratio(float(np.abs(got[k].numpy().astype(np.float64) - w64[i][k]).max()),
                                max(float(np.abs(w32c[i][k] - w64[i][k]).max()), float(np.abs(w32d[i][k] - w64[i][k]).max()))) for k in sd}
            worst = max(ratios.values())
            print("step %d %-8s loss %.9g (float64 %.9g, torch32 error cpu %.3e device %.3e, own error %.3e), weights at most %.2f x torch32's error (%s)" % (
                i, name, mse, l64[i], abs(l32c[i] - l64[i]), abs(l32d[i] - l64[i]), abs(mse - l64[i]), worst, max(ratios, key=ratios.get)))
            assert int(count) == n and e_loss > 0 and abs(mse - l64[i]) <= TOL_FACTOR * e_loss, (i, name)
            assert worst <= TOL_FACTOR, (i, name, worst)
    assert np.isfinite(l64).all()


@pytest.mark.parametrize("two", [True, False], ids=["mlp1", "plain"])
def test_refresh_gives_the_decisions_of_a_fresh_network(two):
    """Three optimizer steps, then refresh_from(trainer): DeviceSarlPolicy.decide on 5 envs of the golden five-adult scene
    gives the bytes (actions, values) of an LstmValueNet freshly built from trainer.state_dict()."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.lstm_rl import LstmValueNet
    from ebcsim.lstm_train import LstmTrainer
    from ebcsim.sarl import DeviceSarlPolicy
    z = load("lstm_interaction_a5" if two else "lstm_plain_a5")
    sd, states, values, _ = _memory(two)
    E = 5
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params_of(z), E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = LstmValueNet(sd, device=DEV)
    policy = DeviceSarlPolicy(net, z["action_space"], 0.9)
    a0, v0 = policy.decide(env)
    v0 = v0.clone()
    tr = LstmTrainer(sd, device=DEV, optimizer="sgd", lr=0.05)
    xs, ys = torch.from_numpy(states).to(DEV), torch.from_numpy(values).to(DEV)
    for _ in range(3):
        tr.loss_and_grad(xs, ys, grad_scale=2.0 / len(values))
        tr.step()
    image = torch.empty(tr.net.packed_floats(), dtype=torch.float32, device=DEV)
    assert torch.equal(tr.net.get_packed(image), tr.flat.detach())  # step() handed the kernel's object the new weights
    assert net.refresh_from(tr) is True and net.native_refreshes == 1
    a1, v1 = policy.decide(env)
    a1, v1 = a1.clone(), v1.clone()
    fresh = LstmValueNet(tr.state_dict(), device=DEV)
    a2, v2 = DeviceSarlPolicy(fresh, z["action_space"], 0.9).decide(env)
    torch.cuda.synchronize()
    assert same_bytes(v1.cpu().numpy(), v2.cpu().numpy()) and same_bytes(a1.cpu().numpy(), a2.cpu().numpy())
    assert not same_bytes(v1.cpu().numpy(), v0.cpu().numpy())  # the steps moved the values
    now = tr.state_dict()
    assert all(torch.equal(v.cpu(), now[k]) for k, v in net.module.state_dict().items())
    assert net.native_forwards > 0
    env.close()


def _generated_env(E, seed_offset=0, missing_penalty=None):
    """E envs of the five-adult config on device-generated train scenes with a restart pool, as tools/train_lstm.py builds them."""
    import configparser
    from ebcsim import actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_lstm.config"))
    if missing_penalty is not None:
        cfg.remove_option("reward", missing_penalty)
    params = ebc_config.params_from_config(cfg, pol)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "train")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    seed0 = ebc_scene.COUNTER_OFFSET["train"] + 100000 * seed_offset
    env.generate_reset(gen, seed0)
    env.generate_pool(gen, seed0 + E, 8 * E)
    return env, ebc_actions.build_action_space(sc.robot.v_pref)


def _fresh_trainer(env, two=True):
    from ebcsim.lstm_train import LstmTrainer
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        return LstmTrainer(module(REFERENCE_NET2 if two else REFERENCE_NET1), device=DEV, optimizer="sgd", lr=0.01)


@pytest.mark.parametrize("two", [True, False], ids=["mlp1", "plain"])
def test_training_schedule_end_to_end(two, tmp_path, monkeypatch):
    """What tools/train_lstm.py runs, small: 64 envs of the five-adult config on generated scenes with a restart pool, 40
    imitation steps and 2 epochs, then 3 RL rounds of 4 optimizer steps: every loss is finite, the weights changed in both
    stages, il_model.pth and rl_model_3.pth load strict, the deciding network was refreshed every round, and every state
    pushed in RL mode has non-increasing `da` over its existing rows."""
    from ebcsim import train as ebc_train
    from ebcsim.lstm_train import DISTANCE_COLUMN, run_lstm_training
    env, space = _generated_env(64)
    assert env.R == 5 and env.T == 13 and all(np.isfinite(float(v)) for v in env.params.collision_penalty)
    tr = _fresh_trainer(env, two)
    start = tr.state_dict()
    pushed, stage = [], {"rl": False}
    push = ebc_train.DeviceReplay.push

    def recording_push(self, states, values, n_valid=None):
        if stage["rl"]:
            pushed.append((states.clone(), None if n_valid is None else n_valid.clone()))
        return push(self, states, values, n_valid)
    monkeypatch.setattr(ebc_train.DeviceReplay, "push", recording_push)
    hist = run_lstm_training(env, tr, space, 0.9, il_steps=40, il_epochs=2, train_iterations=3, steps_per_iteration=4, train_batches=4,
                             batch_size=32, capacity=8192, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=2,
                             generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path),
                             after_il=lambda h: stage.update(rl=True))
    torch.cuda.synchronize()
    print(hist)
    assert hist["il_stored"] > 0 and hist["il_loss"] is not None and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 3 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["native_refreshes"] == 3 and hist["native_forwards"] > 0
    files = {}
    for name in ("il_model.pth", "rl_model_3.pth"):
        files[name] = torch.load(str(tmp_path / name), map_location="cpu")
        module(REFERENCE_NET2 if two else REFERENCE_NET1).load_state_dict(files[name], strict=True)
        assert all(bool(torch.isfinite(v).all()) for v in files[name].values())
    assert not all(torch.equal(files["il_model.pth"][k], start[k]) for k in start)       # imitation moved the weights
    assert not all(torch.equal(files["rl_model_3.pth"][k], files["il_model.pth"][k]) for k in start)  # and so did RL
    assert all(torch.equal(files["rl_model_3.pth"][k], v) for k, v in tr.state_dict().items())
    seen = 0
    for states, nv in pushed:
        da = states[:, :, DISTANCE_COLUMN]
        ok = da[:, 1:] <= da[:, :-1]
        if nv is not None:
            ok = ok | (torch.arange(1, states.shape[1], device=states.device)[None, :] >= nv[:, None])
        assert bool(ok.all())
        seen += int(states.shape[0])
    assert seen > 0  # episodes ended inside the three rounds and went to the memory sorted
    env.close()


def test_a_missing_collision_penalty_stops_the_training(tmp_path):
    """The same schedule on a config without collision_penalty_adult: a collision's reward is NaN, so the imitation
    stage's targets hold a NaN; run_lstm_training raises FloatingPointError before an optimizer step has seen it, the
    weights are the starting ones and no file is written.  Precondition, established on the complete config: the robot
    on ORCA, invisible to the adults, does collide inside the imitation window of these scenes (the first scene seed
    offset at which it does is taken: the dynamics do not depend on the penalty's value)."""
    from ebcsim.lstm_train import run_lstm_training
    from ebcsim.train import DeviceReplay, collect_il
    offset = None
    for cand in range(8):
        env, space = _generated_env(64, cand)
        mem = DeviceReplay(8192, env.R, env.T, torch.device(DEV))
        collect_il(env, mem, 40, 0.9, 0.15)
        collided = bool((mem.values[:len(mem)] == float(env.params.collision_penalty[0])).any())
        env.close()
        if collided:
            offset = cand
            break
    assert offset is not None, "no collision in the imitation window of 8 x 64 scenes"
    env, space = _generated_env(64, offset, missing_penalty="collision_penalty_adult")
    assert np.isnan(float(env.params.collision_penalty[0]))
    tr = _fresh_trainer(env)
    start = tr.state_dict()
    with pytest.raises(FloatingPointError) as err:
        run_lstm_training(env, tr, space, 0.9, il_steps=40, il_epochs=2, train_iterations=3, steps_per_iteration=4, train_batches=4,
                          batch_size=32, capacity=8192, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=2,
                          generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path))
    assert "value target" in str(err.value)
    assert all(torch.equal(v, start[k]) for k, v in tr.state_dict().items()) and not list(tmp_path.iterdir())
    env.close()
