"""The layer form of the SARL gradient (ebc_sarl_net_create_layers; csrc/ebc_sarl_grad_layers.h) on the device: every
output (grad, loss_sum, count, value, attention) against the wide host build of the same rule
(tests/native/sarl_grad_layers_host.cc), byte for byte, every output poisoned before each call: the narrow networks over
the chunk form's own matrix of batches, the reference widths (also against the chunk kernel on the same device), a
network whose widths sit on both sides of the 32- and 64-wide tiles, the x2 and x4 widths, wide rows, row counts past every
LDS limit of the chunk form, more row slots than one run takes, NaN / dead / empty batches, subnormal products, canaries,
the refusals; SarlFormTrainer(grad_form=...); and the training schedule on the x2 network.  Cases: tests/sarl_grad_cases.py and
tests/sarl_grad_layers_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sarl_grad_cases import (BATCHES, NETS, REFERENCE_NET, ROWS, TOL_FACTOR, chunk, edge_batch, module, plain_batch, random_state_dict, same_bytes)
from sarl_grad_layers_cases import EDGE_NET, X2_NET, X4_NET, constant, host_grad, host_pack
from ebcsim import _abi, _capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xB6
NARROW = NETS[1]

_nets = {}


def device_net(net, om_width=0, form="layers"):
    """(state_dict, packed image by the wide host build's pack, SarlNet of `form` on the device) of a seeded network, once."""
    key = (tuple(net[0]), net[2], om_width, form)
    if key not in _nets:
        from ebcsim.sarl_train import SarlNet
        sd = random_state_dict(net)
        _nets[key] = (sd, host_pack(sd, om_width), SarlNet(sd, 0, om_width=om_width or None, form=form))
    return _nets[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_grad(dn, rows, target, nv, mask, scale):
    """(grad, loss_sum, count, value, attention) of one ebc_sarl_grad on host arrays, every output poisoned before."""
    B, R, _ = rows.shape
    grad = torch.full((dn.packed_floats(),), -7.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -7.0, dtype=torch.float64, device=DEV), torch.full((), -7, dtype=torch.int64, device=DEV)
    value, att = torch.full((B,), -7.0, dtype=torch.float32, device=DEV), torch.full((B, R), -7.0, dtype=torch.float32, device=DEV)
    dn.grad(_dev(rows), _dev(target), grad, loss, count, scale, _dev(nv), _dev(mask), value, att)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), att.cpu().numpy()


def assert_same(got, want, tag):
    assert same_bytes(got[0], want[0]), (tag, "grad", np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (tag, "loss_sum", got[1], want[1])
    assert got[2] == want[2], (tag, "count", got[2], want[2])
    assert same_bytes(got[3], want[3]), (tag, "value", got[3], want[3])
    assert same_bytes(got[4], want[4]), (tag, "attention", got[4], want[4])


def check(net, B, R, om_width=0, edge=True, seed=None):
    """A plain batch, and with `edge` the edge batch with and without its mask, against the wide host build."""
    sd, P, dn = device_net(net, om_width)
    rows, target = plain_batch(net, B, R, seed)
    assert_same(kernel_grad(dn, rows, target, None, None, 2.0 / B), host_grad(P, net, rows, target, None, None, 2.0 / B, om_width), ("plain", B, R))
    if not edge:
        return
    rows, target, nv, mask, kinds = edge_batch(net, B, R, seed)
    assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), host_grad(P, net, rows, target, nv, mask, 2.0 / B, om_width), ("edge", B, R, kinds))
    assert_same(kernel_grad(dn, rows, target, nv, None, 2.0 / B), host_grad(P, net, rows, target, nv, None, 2.0 / B, om_width), ("no mask", B, R))


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("ni", [1, 2, 3], ids=["narrow", "narrow_rows_17", "narrow_no_global_state"])
def test_layer_form_equals_host_build_bytes(ni, R):
    """The matrix of tests/test_sarl_train_gpu.py's kernel test on the layer form: B in 1, C - 1, C, C + 1, 2 C + 1, plain,
    edge with mask, edge without mask, and a second call on the same inputs; the packed image is the header's."""
    net = NETS[ni]
    sd, P, dn = device_net(net)
    image = torch.empty(dn.packed_floats(), dtype=torch.float32, device=DEV)
    assert same_bytes(dn.get_packed(image).cpu().numpy(), P)
    for B in BATCHES:
        check(net, B, R)
        rows, target, nv, mask, _ = edge_batch(net, B, R)
        got = kernel_grad(dn, rows, target, nv, mask, 2.0 / B)
        assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), got, ("again", B, R))


@pytest.mark.parametrize("B,R", [(5, 5), (9, 10)])
def test_reference_widths_equal_host_build_and_chunk_kernel(B, R):
    """At the reference widths both forms take the network: the layer form's bytes are the host build's and the chunk
    kernel's on the same device; a flat weight tensor passes from one form's network to the other's."""
    check(REFERENCE_NET, B, R)
    sd, P, layers = device_net(REFERENCE_NET)
    _, _, chunked = device_net(REFERENCE_NET, form="chunk")
    assert layers.packed_floats() == chunked.packed_floats()
    rows, target, nv, mask, _ = edge_batch(REFERENCE_NET, B, R)
    assert_same(kernel_grad(layers, rows, target, nv, mask, 2.0 / B), kernel_grad(chunked, rows, target, nv, mask, 2.0 / B), ("forms", B, R))
    image = torch.empty(chunked.packed_floats(), dtype=torch.float32, device=DEV)
    other = (chunked.get_packed(image) * 0.5).contiguous()
    try:
        layers.set_packed(other)
        chunked.set_packed(other)
        assert_same(kernel_grad(layers, rows, target, nv, mask, 2.0 / B), kernel_grad(chunked, rows, target, nv, mask, 2.0 / B), ("handed on", B, R))
    finally:
        layers.set_packed(_dev(P))
        chunked.set_packed(_dev(P))
        torch.cuda.synchronize()


@pytest.mark.parametrize("B,R", [(5, 3), (9, 33)])
def test_widths_on_both_sides_of_the_tiles(B, R):
    check(EDGE_NET, B, R)


@pytest.mark.parametrize("name,B,R", [("x2", 1, 1), ("x2", 5, 5), ("x2", 9, 30), ("x4", 5, 2)])
def test_wide_networks(name, B, R):
    check(X2_NET if name == "x2" else X4_NET, B, R)


@pytest.mark.parametrize("T,W", [(13, 52), (32, 192)], ids=["65_columns", "224_columns"])
def test_wide_rows(T, W):
    """OM rows: the narrow network with mlp1.0 on T + W columns, om_width = W."""
    net = ([T + W] + NARROW[0][1:], 6, True)
    check(net, 5, 3, om_width=W)


@pytest.mark.parametrize("R", [33, 128])
def test_row_counts_past_the_chunk_forms_limits(R):
    sd, P, dn = device_net(NARROW)
    assert dn.grad_max_rows() == constant("max_rows") == 128 and dn.grad_max_rows(0) == 128
    check(NARROW, 5, R)


def test_more_row_slots_than_one_run_takes():
    """B * R just above EBC_SARL_GRAD_LAYERS_RUN_SLOTS at R = 16 with ragged n_valid and a mask: the second run continues
    the float64 sums of the first."""
    R = 16
    B = constant("run_slots") // R + chunk() + 1
    sd, P, dn = device_net(NARROW)
    rows, target = plain_batch(NARROW, B, R, seed=91)
    nv = (np.arange(B) * 7 % (R + 3) - 1).astype(np.int64)  # -1 .. R + 1
    mask = (np.arange(B) % 5 != 2).astype(np.uint8)
    assert_same(kernel_grad(dn, rows, target, nv, mask, 2.0 / B), host_grad(P, NARROW, rows, target, nv, mask, 2.0 / B), "two runs")


def test_a_nan_in_a_live_row_a_batch_without_live_states_and_an_empty_batch():
    sd, P, dn = device_net(NARROW)
    rows, target = plain_batch(NARROW, 7, 2, seed=81)
    rows[5, 1, 3] = np.nan
    want = host_grad(P, NARROW, rows, target, None, None, 0.1)
    assert np.isnan(want[1]) and np.isnan(want[0]).any()
    assert_same(kernel_grad(dn, rows, target, None, None, 0.1), want, "nan")
    mask = np.zeros(7, dtype=np.uint8)
    got = kernel_grad(dn, rows, target, None, mask, 0.1)
    assert_same(got, host_grad(P, NARROW, rows, target, None, mask, 0.1), "dead")
    assert got[2] == 0 and got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()
    got = kernel_grad(dn, rows[:0], target[:0], None, None, 0.1)
    assert got[2] == 0 and got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()


def test_subnormal_products():
    """Rows and targets times 2^-70: the matrix instruction's C / D never flush and its A / B follow the kernel's denormal
    mode, which keeps them; with a grad_scale of 2^-60 on top, layer 0's products delta * x are subnormal (the host build's
    gradient holds subnormal entries: checked), and the bytes are still the host build's."""
    sd, P, dn = device_net(NARROW)
    rows, target = plain_batch(NARROW, 9, 5, seed=92)
    rows, target = (rows * np.float32(2.0 ** -70)).astype(np.float32), (target * np.float32(2.0 ** -70)).astype(np.float32)
    assert_same(kernel_grad(dn, rows, target, None, None, 2.0 / 9), host_grad(P, NARROW, rows, target, None, None, 2.0 / 9), "2^-70")
    want = host_grad(P, NARROW, rows, target, None, None, 2.0 ** -60)
    tiny = np.abs(want[0][want[0] != 0])
    assert (tiny < np.finfo(np.float32).tiny).any()
    assert_same(kernel_grad(dn, rows, target, None, None, 2.0 ** -60), want, "subnormal")


@pytest.mark.parametrize("B,R", [(9, 5), (33, 3)])
def test_guard_words_around_the_outputs(B, R):
    """grad, value and attention as slices of larger tensors filled with a canary, at row counts (45 and 99 slots, 9 and 33
    states) that leave lanes and waves of the last tiles without a row."""
    sd, P, dn = device_net(NARROW)
    PF, pad = dn.packed_floats(), 4096
    rows, target, nv, mask, _ = edge_batch(NARROW, B, R)
    raw = {k: torch.full((2 * pad + n * 4,), CANARY, dtype=torch.uint8, device=DEV)
           for k, n in (("grad", PF), ("value", B), ("attention", B * R), ("loss", 2), ("count", 2))}
    inside = {k: v[pad:v.numel() - pad] for k, v in raw.items()}
    grad, value, att = inside["grad"].view(torch.float32), inside["value"].view(torch.float32), inside["attention"].view(torch.float32)
    loss, count = inside["loss"].view(torch.float64).reshape(()), inside["count"].view(torch.int64).reshape(())
    dn.grad(_dev(rows), _dev(target), grad, loss, count, 2.0 / B, _dev(nv), _dev(mask), value, att)
    torch.cuda.synchronize()
    for k, v in raw.items():
        b = v.cpu().numpy()
        assert (b[:pad] == CANARY).all() and (b[-pad:] == CANARY).all(), k
    assert_same((grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), att.cpu().numpy().reshape(B, R)),
                host_grad(P, NARROW, rows, target, nv, mask, 2.0 / B), "guarded")


def _create_layers(widths, om_width=0, self_dim=6):
    """ebc_sarl_net_create_layers on zero weights of the given shape -> (rc, handle, message)."""
    w = _abi.EbcSarlNetWeights()
    w.struct_size = C.sizeof(w)
    w.n_mlp1, w.n_mlp2, w.n_attention, w.n_mlp3 = 2, 2, 3, 4
    w.with_global_state, w.self_state_dim, w.input_dim = 1, self_dim, widths[0]
    keep = []
    for i, v in enumerate(widths[1:]):
        w.widths[i] = v
        keep.append((np.zeros((max(v, 1), 1300), dtype=np.float32), np.zeros((max(v, 1),), dtype=np.float32)))
        w.weight[i], w.bias[i] = keep[-1][0].ctypes.data, keep[-1][1].ctypes.data
    h = C.c_void_p()
    rc = _capi.lib().ebc_sarl_net_create_layers(C.addressof(w), om_width, 0, C.byref(h))
    return rc, h, _capi.lib().ebc_last_error()


def test_refusals_leave_every_output_untouched():
    """641 units, R = 129, R = 0, states_per_pass = 2 (and 3), a wrong T and a capturing stream: refused by name with the
    right code, nothing written, and the entry stays usable."""
    lib = _capi.lib()
    rc, h, msg = _create_layers([13, 641, 100, 100, 50, 100, 100, 1, 150, 100, 100, 1])
    assert rc == _abi.ERR_UNSUPPORTED and b"1 .. 640" in msg and not h.value, msg
    rc, h, msg = _create_layers([13, 150, 100, 100, 50, 100, 100, 2, 150, 100, 100, 1])
    assert rc == _abi.ERR_UNSUPPORTED and b"exactly 1" in msg and not h.value, msg
    rc, h, msg = _create_layers([33, 150, 100, 100, 50, 100, 100, 1, 150, 100, 100, 1], om_width=192)
    assert rc == _abi.ERR_UNSUPPORTED and b"224" in msg and not h.value, msg
    rc, h, msg = _create_layers([64] + [640] * 6 + [1] + [640] * 3 + [1])  # the limits themselves are taken
    assert rc == _abi.OK and h.value
    rows_out = C.c_int(-1)
    assert lib.ebc_sarl_net_grad_max_rows(h, C.byref(rows_out)) == _abi.OK and rows_out.value == 128
    assert lib.ebc_sarl_net_grad_max_rows_at(h, 0, C.byref(rows_out)) == _abi.OK and rows_out.value == 128
    for S in (4, 2, 1):
        assert lib.ebc_sarl_net_grad_max_rows_at(h, S, C.byref(rows_out)) == _abi.ERR_UNSUPPORTED and b"no passes" in lib.ebc_last_error()
    assert lib.ebc_sarl_net_grad_max_rows_at(h, 3, C.byref(rows_out)) == _abi.ERR_INVALID
    assert lib.ebc_sarl_net_destroy(h) == _abi.OK

    sd, P, dn = device_net(NARROW)
    T = NARROW[0][0]
    rows, target = plain_batch(NARROW, 3, 2, seed=83)
    want = host_grad(P, NARROW, rows, target, None, None, 1.0)
    grad = torch.full((dn.packed_floats(),), -5.0, dtype=torch.float32, device=DEV)
    loss, count = torch.full((), -5.0, dtype=torch.float64, device=DEV), torch.full((), -5, dtype=torch.int64, device=DEV)

    def refused(R, Tr, sp, code, word):
        value, att = torch.full((2,), -5.0, dtype=torch.float32, device=DEV), torch.full((2, max(R, 1)), -5.0, dtype=torch.float32, device=DEV)
        a = _abi.EbcSarlGradArgs()
        a.struct_size = C.sizeof(a)
        a.B, a.R, a.T, a.grad_scale, a.states_per_pass = 2, R, Tr, 1.0, sp
        x, y = torch.zeros((2, max(R, 1), Tr), dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV)
        a.rows, a.target, a.grad, a.loss_sum, a.count = x.data_ptr(), y.data_ptr(), grad.data_ptr(), loss.data_ptr(), count.data_ptr()
        a.value, a.attention = value.data_ptr(), att.data_ptr()
        rc = lib.ebc_sarl_grad(dn._h, torch.cuda.current_stream().cuda_stream, C.addressof(a))
        assert rc == code and word in lib.ebc_last_error(), (R, Tr, sp, rc, lib.ebc_last_error())
        torch.cuda.synchronize()
        assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5 and bool((value == -5.0).all()) and bool((att == -5.0).all())
    refused(129, T, 0, _abi.ERR_UNSUPPORTED, b"R = 129")
    refused(0, T, 0, _abi.ERR_UNSUPPORTED, b"R < 1")
    refused(2, T, 2, _abi.ERR_UNSUPPORTED, b"no passes")
    refused(2, T, 3, _abi.ERR_INVALID, b"states_per_pass")
    refused(2, T + 1, 0, _abi.ERR_INVALID, b"wide")

    rd, td = _dev(rows), _dev(target)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dn.grad(rd, td, grad, loss, count, 1.0)  # the scratch is there before the capture
        side.synchronize()
        grad.fill_(-5.0)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError) as err:
                dn.grad(rd, td, grad, loss, count, 1.0)
        finally:
            graph.capture_end()
        assert err.value.code == _abi.ERR_UNSUPPORTED and "captured" in str(err.value)
        side.synchronize()
        assert bool((grad == -5.0).all())
        dn.grad(rd, td, grad, loss, count, 1.0)
        side.synchronize()
    assert same_bytes(grad.cpu().numpy(), want[0]) and float(loss) == want[1] and int(count) == want[2]


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_forms_take_the_same_steps_at_the_reference_widths():
    """Three SGD steps on the golden memory: SarlFormTrainer(grad_form="layers") and grad_form=None leave the same bytes in
    every step's loss, count and master copy; "auto" takes the chunk form at R = 5 and the layer form at R = 30."""
    from ebcsim.sarl_train import SarlFormTrainer, SarlTrainer
    from test_sarl_train_gpu import _golden_memory
    sd, states, values, lr = _golden_memory()
    trainers = [SarlFormTrainer(sd, device=DEV, optimizer="sgd", lr=lr, grad_form=f) for f in (None, "layers", "auto")]
    assert [t.net.form for t in trainers] == ["chunk", "layers", "chunk"]
    assert trainers[1].grad_max_rows() == 128 and trainers[2].grad_max_rows() == 128 and trainers[0].grad_max_rows() < 30
    xs, ys = torch.from_numpy(states).to(DEV), torch.from_numpy(values).to(DEV)
    assert xs.shape[1] == 5
    for i in range(3):
        outs = []
        for t in trainers:
            loss, count = t.loss_and_grad(xs, ys, grad_scale=2.0 / len(values))
            t.step()
            outs.append((float(loss), int(count), t.flat.detach().cpu().numpy()))
        for o in outs[1:]:
            assert np.float64(o[0]).tobytes() == np.float64(outs[0][0]).tobytes() and o[1] == outs[0][1] and same_bytes(o[2], outs[0][2]), i
    auto = trainers[2]
    assert auto.form_of(5) == "chunk" and auto.form_of(30) == "layers" and auto.net.layers is None and auto.net.chunk is not None
    x30 = torch.zeros((len(values), 30, xs.shape[2]), device=DEV)
    x30[:, :5] = xs
    nv = torch.full((len(values),), 5, dtype=torch.int64, device=DEV)
    loss30, _ = auto.loss_and_grad(x30, ys, n_valid=nv, grad_scale=2.0 / len(values))
    assert auto.net.layers is not None and auto.net.form == "layers"
    g30 = auto.flat.grad.clone()
    loss5, _ = auto.loss_and_grad(xs, ys, grad_scale=2.0 / len(values))
    assert auto.net.form == "chunk"
    # five rows of thirty are the five rows: the layer form at R = 30 and the chunk form at R = 5 on the same states
    assert torch.equal(g30, auto.flat.grad) and float(loss30) == float(loss5)
    auto.step()  # push_weights reaches both network objects
    for net in (auto.net.chunk, auto.net.layers):
        assert torch.equal(net.get_packed(torch.empty_like(auto.flat.detach())), auto.flat.detach())


def test_trainer_at_the_x2_widths():
    """SarlTrainer(x2, native=True), the chunk form, still raises; "auto" and "layers" take the layer form; three SGD
    steps of grad_form="layers" stay, per tensor and in the loss, within TOL_FACTOR times torch's float32 error (the
    larger of its CPU and device forms against the same steps in float64) of those float64 steps, as native=False does."""
    from ebcsim.sarl_train import SarlFormTrainer, SarlTrainer
    from test_sarl_train_gpu import _float64_steps, _ratio
    sd = random_state_dict(X2_NET)
    with pytest.raises(_capi.EbcError) as err:
        SarlTrainer(sd, device=DEV, native=True)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "1 .. 256" in str(err.value)
    auto = SarlFormTrainer(sd, device=DEV, grad_form="auto")
    assert auto.net.chunk is None and auto.net.layers is not None and auto.net.form == "layers" and auto.form_of(5) == "layers"
    states, values = plain_batch(X2_NET, 64, 5, seed=93)
    lr, steps = 0.01, 3
    (l64, w64), (l32c, w32c), (l32d, w32d) = (lambda r: (r["f64"], r["f32_cpu"], r["f32_dev"]))(_float64_steps(sd, states, values, lr, steps))
    trainers = {"layers": SarlFormTrainer(sd, device=DEV, optimizer="sgd", lr=lr, grad_form="layers"),
                "autograd": SarlFormTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=False, grad_form="layers")}
    assert trainers["layers"].native and not trainers["autograd"].native and trainers["autograd"].net is None
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
            print("step %d %-8s loss %.9g (float64 %.9g, torch32 error %.3e, own %.3e), weights at most %.2f x torch32's error (%s)" % (
                i, name, mse, l64[i], e_loss, abs(mse - l64[i]), worst, max(ratios, key=ratios.get)))
            assert int(count) == n and e_loss > 0 and abs(mse - l64[i]) <= TOL_FACTOR * e_loss, (i, name)
            assert worst <= TOL_FACTOR, (i, name, worst)


def test_training_schedule_on_the_x2_network(tmp_path):
    """run_sarl_training with the x2 network on sarl_a5.config and device scenes, small: 8 envs, 1 imitation epoch, 2 RL
    rounds.  The imitation window is 60 steps, not 3: the memory takes the states of episodes that END inside the window,
    and none of these scenes' episodes ends in 3 steps, which would leave nothing to train on.  Losses are finite, the
    deciding blocks were refreshed from the trainer, and the saved file loads into SarlModule with strict=True."""
    from ebcsim.sarl import SarlValueNet
    from ebcsim.sarl_train import SarlFormTrainer, SarlTrainer, run_sarl_training
    from test_sarl_train_gpu import _generated_env
    env, space = _generated_env(8)
    net = ([env.T] + X2_NET[0][1:], 6, True)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(12)
        tr = SarlFormTrainer(module(net), device=DEV, optimizer="sgd", lr=0.01, grad_form="auto")
    assert tr.net.form == "layers"
    start = tr.state_dict()
    hist = run_sarl_training(env, tr, space, 0.9, il_steps=60, il_epochs=1, train_iterations=2, steps_per_iteration=2, train_batches=2,
                             batch_size=16, capacity=2048, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=1,
                             generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path))
    torch.cuda.synchronize()
    print(hist)
    assert hist["il_stored"] > 0 and hist["il_loss"] is not None and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 2 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["native_refreshes"] > 0
    saved = torch.load(str(tmp_path / "rl_model_2.pth"), map_location="cpu")
    module(net).load_state_dict(saved, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in saved.values())
    assert not all(torch.equal(saved[k], start[k]) for k in start)
    # the deciding network takes the x2 widths: its values on a few states are the module's, to the blocks' accuracy
    fresh = SarlValueNet(tr.state_dict(), device=DEV, with_global_state=True, self_state_dim=6)
    m = module(net)
    m.load_state_dict(saved, strict=True)
    x = torch.from_numpy(plain_batch(net, 6, env.R, seed=94)[0])
    with torch.no_grad():
        want = m(x, None)
    got = fresh.forward(x.to(DEV)).cpu()
    assert bool(torch.isfinite(got).all()) and float((got - want).abs().max()) <= 1e-3
    env.close()
