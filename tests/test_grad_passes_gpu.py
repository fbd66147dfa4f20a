"""The pass form of the two gradient kernels (EbcSarlGradArgs.states_per_pass / EbcLstmGradArgs.states_per_pass: a chunk's 4
states run 4, 2 or 1 at a time, so that more rows per state fit a workgroup's LDS).  The host builds of the unchanged rule
headers are the reference at every shape: the bytes must not depend on the pass size, below the whole chunk's row limit
(where they are also the default call's) and above it; the bookkeeping at chunk edges; the limits and the refusals; the
trainers and the schedules with states_per_pass="auto".  Cases: tests/sarl_grad_cases.py, tests/lstm_grad_cases.py,
tests/om_train_cases.py, tests/om_lstm_cases.py."""
import configparser
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lstm_grad_cases as lg
import om_lstm_cases as ol
import om_train_cases as oc
import sarl_grad_cases as sg
from cadrl_cases import TOL_FACTOR
from ebcsim import _abi, _capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xB6
PASSES = (4, 2, 1)
ROOT = sg.ROOT


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Kit(object):
    """One kernel's side of a comparison: its seeded network on the device, the host build, the last output's shape."""

    def __init__(self, kind, net, sd, P, dn, host_grad, cases):
        self.kind, self.net, self.sd, self.P, self.dn, self._host, self.cases = kind, net, sd, P, dn, host_grad, cases

    def extra_shape(self, B, R):
        return (B, R) if self.kind == "sarl" else (B, self.dn.joint_dim)

    def outputs(self, B, R, poison=-7.0):
        return (torch.full((self.dn.packed_floats(),), poison, dtype=torch.float32, device=DEV),
                torch.full((), poison, dtype=torch.float64, device=DEV), torch.full((), int(poison), dtype=torch.int64, device=DEV),
                torch.full((B,), poison, dtype=torch.float32, device=DEV),
                torch.full(self.extra_shape(B, R), poison, dtype=torch.float32, device=DEV))

    def kernel(self, rows, target, nv, mask, scale, S):
        """(grad, loss_sum, count, value, attention / joint) of one call with states_per_pass = S, every output poisoned before."""
        B, R, _ = rows.shape
        grad, loss, count, value, extra = self.outputs(B, R)
        self.dn.grad(_dev(rows), _dev(target), grad, loss, count, scale, _dev(nv), _dev(mask), value, extra, states_per_pass=S)
        torch.cuda.synchronize()
        return grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), extra.cpu().numpy()

    def host(self, rows, target, nv, mask, scale):
        return self._host(self.P, self.net, rows, target, nv, mask, scale)


_kits = {}


def kit(kind, ni):
    """kind "sarl": sg.NETS[ni]; "lstm": lg.NETS[ni]; "om_sarl": the 65-wide reference network; "om_lstm": ol.GRAD_NETS[ni]."""
    if (kind, ni) not in _kits:
        from ebcsim.lstm_train import LstmNet
        from ebcsim.sarl_train import SarlNet
        if kind == "sarl":
            net, sd = sg.NETS[ni], sg.random_state_dict(sg.NETS[ni])
            k = Kit("sarl", net, sd, sg.host_pack(sd), SarlNet(sd, 0), sg.host_grad, sg)
        elif kind == "om_sarl":
            wnet = oc.REFERENCE_WIDE_65
            sd = sg.random_state_dict(wnet[0])
            k = Kit("sarl", wnet, sd, oc.host_pack(sd, wnet[1]), SarlNet(sd, 0, om_width=wnet[1]), oc.host_grad, sg)
        else:
            net = lg.NETS[ni] if kind == "lstm" else ol.GRAD_NETS[ni]
            sd = lg.random_state_dict(net, scale=4.0 if net[0][5] == 7 else 1.0)
            k = Kit("lstm", net, sd, lg.host_pack(sd), LstmNet(sd, 0), lg.host_grad, lg)
        _kits[kind, ni] = k
    return _kits[kind, ni]


def assert_same(got, want, tag):
    assert sg.same_bytes(got[0], want[0]), (tag, "grad", np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (tag, "loss_sum", got[1], want[1])
    assert got[2] == want[2], (tag, "count", got[2], want[2])
    assert sg.same_bytes(got[3], want[3]), (tag, "value", got[3], want[3])
    assert sg.same_bytes(got[4], want[4]), (tag, "attention / joint", got[4], want[4])


NARROW = [("sarl", 1), ("sarl", 2), ("sarl", 3), ("lstm", 2), ("lstm", 3)]
NARROW_IDS = ["sarl_narrow", "sarl_narrow_rows_17", "sarl_narrow_no_global_state", "lstm_narrow_mlp1", "lstm_narrow_plain"]


# ------------------------------------------------------------------------------- 1. the bytes do not depend on S
@pytest.mark.parametrize("R", [1, 2, 3, 5])
@pytest.mark.parametrize("kind,ni", NARROW, ids=NARROW_IDS)
def test_bytes_do_not_depend_on_the_pass_size(kind, ni, R):
    """Narrow networks, B in 1 .. 5 and 9, plain batches and the edge batches (ragged n_valid) with a mask and without: with
    states_per_pass 4, 2 and 1 every output is the host build's, byte for byte, and so the default call's (asserted too); a
    second call gives the same bytes."""
    k = kit(kind, ni)
    for B in (1, 2, 3, 4, 5, 9):
        rows, target = k.cases.plain_batch(k.net, B, R)
        erows, etarget, nv, mask, kinds = k.cases.edge_batch(k.net, B, R)
        for tag, args in (("plain", (rows, target, None, None)), ("edge", (erows, etarget, nv, mask)), ("no mask", (erows, etarget, nv, None))):
            want = k.host(*args, 2.0 / B)
            assert_same(k.kernel(*args, 2.0 / B, 0), want, (tag, B, R, "default"))
            for S in PASSES:
                assert_same(k.kernel(*args, 2.0 / B, S), want, (tag, B, R, S, kinds))
        for S in PASSES:
            assert_same(k.kernel(erows, etarget, nv, mask, 2.0 / B, S), k.host(erows, etarget, nv, mask, 2.0 / B), ("again", B, R, S))


# ------------------------------------------------------------------------------- 2. pass bookkeeping at chunk edges
EDGE_MASKS = {
    "only_the_last_state_of_a_chunk_is_live": ([0, 0, 0, 1, 0, 0, 0, 1, 1], None),
    "first_and_last_live_dead_between": ([1, 0, 0, 1, 1, 0, 0, 1, 1], None),
    "a_dead_chunk_between_two_live_ones": ([1, 1, 1, 1, 0, 0, 0, 0, 1], None),
    "no_rows_in_the_first_pass": (None, [0, -1, 3, 2, -2, 0, 1, 3, 0]),
    "no_rows_in_the_first_pass_and_a_mask": ([1, 1, 0, 1, 1, 1, 1, 0, 1], [0, -1, 3, 2, -2, 0, 1, 3, 0]),
}


@pytest.mark.parametrize("case", sorted(EDGE_MASKS))
@pytest.mark.parametrize("kind,ni", [("sarl", 1), ("lstm", 2)], ids=["sarl", "lstm"])
def test_pass_bookkeeping_at_chunk_edges(kind, ni, case):
    """B = 9, R = 3: the first live state of a chunk lies in a later pass (the partial must have been started from 0 all the
    same), dead states between live ones, a chunk without a live state (zeros), states without rows in the first pass."""
    k = kit(kind, ni)
    mask, nv = EDGE_MASKS[case]
    mask = None if mask is None else np.array(mask, dtype=np.uint8)
    nv = None if nv is None else np.array(nv, dtype=np.int64)
    rows, target = k.cases.plain_batch(k.net, 9, 3, seed=4100 + len(case))
    want = k.host(rows, target, nv, mask, 0.3)
    assert want[2] == int(sg.is_live(np.full(9, 3) if nv is None else nv, np.ones(9) if mask is None else mask).sum()) > 0
    for S in (0,) + PASSES:
        assert_same(k.kernel(rows, target, nv, mask, 0.3, S), want, (case, S))


# ------------------------------------------------------------------------------- 3. the new ground
def ragged(B, R):
    """n_valid holding R, 1, R + 3 and an odd count below R."""
    odd = R - 1 if (R - 1) % 2 else R - 2
    return np.array(([R, 1, R + 3, max(odd, 1), R - 2] * 2)[:B], dtype=np.int64)


def test_limits_come_from_the_lds_and_grow_as_the_pass_shrinks():
    """grad_max_rows(4) is the whole chunk's; 2 and 1 states at a time take about twice and four times the rows: at the
    reference widths SARL past 30 with S = 2, the 65-wide network and LSTM with mlp1 with S = 1 (the 30-row scenes)."""
    for key in (("sarl", 0), ("om_sarl", 0), ("lstm", 0), ("lstm", 1), ("om_lstm", 2), ("om_lstm", 3), ("sarl", 1), ("lstm", 2)):
        dn = kit(*key).dn
        whole, m4, m2, m1 = dn.grad_max_rows(), dn.grad_max_rows(4), dn.grad_max_rows(2), dn.grad_max_rows(1)
        print(key, whole, m4, m2, m1)
        assert whole == dn.grad_max_rows(0) == m4 and 2 * m4 <= m2 <= 2 * m4 + 4 and 2 * m2 <= m1 <= 2 * m2 + 4, key
    assert kit("sarl", 0).dn.grad_max_rows(2) >= 30 and kit("om_sarl", 0).dn.grad_max_rows(1) >= 30
    assert kit("lstm", 0).dn.grad_max_rows(1) >= 33 and kit("lstm", 1).dn.grad_max_rows(2) >= 33


NEW_GROUND = [("sarl", 0, 5, 16, 2), ("sarl", 0, 5, 17, 2), ("sarl", 0, 9, 30, 1), ("sarl", 0, 5, 31, 1), ("om_sarl", 0, 5, 30, 1),
              ("om_sarl", 0, 5, 15, 2), ("lstm", 0, 5, 13, 2), ("lstm", 0, 5, 14, 2), ("lstm", 0, 9, 30, 1), ("lstm", 0, 5, 31, 1),
              ("lstm", 1, 5, 27, 2), ("lstm", 1, 5, 28, 2), ("om_lstm", 2, 5, 30, 1), ("om_lstm", 3, 5, 30, 1), ("om_lstm", 3, 5, 29, 1)]


@pytest.mark.parametrize("kind,ni,B,R,S", NEW_GROUND, ids=["%s%d_B%d_R%d_S%d" % c for c in NEW_GROUND])
def test_rows_past_the_whole_chunk_at_the_reference_widths(kind, ni, B, R, S):
    """Reference widths, R above what the whole chunk takes, an odd and an even R per kernel and pass size (SC, WT and the
    per-state arrays are S * R or S floats long: what follows them must stay aligned): the host build's bytes with ragged
    n_valid (R, 1, R + 3, an odd count) and a mask, and the default call refuses this R."""
    k = kit(kind, ni)
    assert k.dn.grad_max_rows() < R <= k.dn.grad_max_rows(S)
    if kind == "om_sarl":
        rows, target = oc.wide_batch(k.net, B, R, seed=7700 + R)
    else:
        rows, target = k.cases.plain_batch(k.net, B, R, seed=7700 + R)
    nv, mask = ragged(B, R), np.array(([1, 1, 1, 0, 1] * 2)[:B], dtype=np.uint8)
    assert_same(k.kernel(rows, target, nv, mask, 2.0 / B, S), k.host(rows, target, nv, mask, 2.0 / B), (kind, ni, B, R, S))
    with pytest.raises(_capi.EbcError) as err:
        k.kernel(rows, target, nv, mask, 2.0 / B, 0)
    assert err.value.code == _abi.ERR_UNSUPPORTED


@pytest.mark.parametrize("S", [2, 1])
@pytest.mark.parametrize("kind,ni", [("sarl", 0), ("lstm", 0), ("lstm", 1), ("om_lstm", 2), ("om_lstm", 3)],
                         ids=["sarl", "lstm_mlp1", "lstm_plain", "om_lstm_mlp1", "om_lstm_plain"])
def test_the_largest_r_of_a_pass_size_runs_and_one_more_is_refused(kind, ni, S):
    """grad_max_rows(S) itself with B = 5: the host build's bytes.  One row more: EBC_ERR_UNSUPPORTED, the message names R, S
    and the limit, and every output still holds its poison."""
    k = kit(kind, ni)
    R, B = k.dn.grad_max_rows(S), 5
    rows, target = k.cases.plain_batch(k.net, B, R, seed=7800 + S)
    nv = ragged(B, R)
    assert_same(k.kernel(rows, target, nv, None, 0.4, S), k.host(rows, target, nv, None, 0.4), (kind, ni, R, S))
    grad, loss, count, value, extra = k.outputs(2, R + 1, poison=-5.0)
    with pytest.raises(_capi.EbcError) as err:
        k.dn.grad(torch.zeros((2, R + 1, k.net[0][0]), dtype=torch.float32, device=DEV), torch.zeros(2, device=DEV), grad, loss, count, 1.0,
                  None, None, value, extra, states_per_pass=S)
    msg = str(err.value)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "R = %d" % (R + 1) in msg and "S = %d" % S in msg and "up to R = %d" % R in msg, msg
    torch.cuda.synchronize()
    assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5 and bool((value == -5.0).all()) and bool((extra == -5.0).all())


# ------------------------------------------------------------------------------- 4. other edge cases
@pytest.mark.parametrize("kind,ni", [("sarl", 1), ("lstm", 2)], ids=["sarl", "lstm"])
def test_a_nan_in_a_live_row_of_a_chunks_first_pass(kind, ni):
    k = kit(kind, ni)
    rows, target = k.cases.plain_batch(k.net, 7, 2, seed=81)
    rows[4, 1, 3] = np.nan  # state 4: the first of the second chunk, its first pass at S = 1
    want = k.host(rows, target, None, None, 0.1)
    assert np.isnan(want[1]) and np.isnan(want[0]).any()
    for S in PASSES:
        assert_same(k.kernel(rows, target, None, None, 0.1, S), want, ("nan", S))


@pytest.mark.parametrize("kind,ni", [("sarl", 1), ("lstm", 2)], ids=["sarl", "lstm"])
def test_guard_words_around_the_outputs_one_state_per_pass(kind, ni):
    """test_guard_words_around_the_outputs at S = 1, R = 5, B = 9: grad, value, attention / joint, loss and count as slices
    of larger tensors filled with a canary; the bytes on both sides are intact, the insides are the host build's."""
    k = kit(kind, ni)
    B, R, PF, pad = 9, 5, k.dn.packed_floats(), 4096
    rows, target, nv, mask, _ = k.cases.edge_batch(k.net, B, R)
    shape = k.extra_shape(B, R)
    raw = {name: torch.full((2 * pad + n * 4,), CANARY, dtype=torch.uint8, device=DEV)
           for name, n in (("grad", PF), ("value", B), ("extra", shape[0] * shape[1]), ("loss", 2), ("count", 2))}
    inside = {name: v[pad:v.numel() - pad] for name, v in raw.items()}
    grad, value, extra = inside["grad"].view(torch.float32), inside["value"].view(torch.float32), inside["extra"].view(torch.float32)
    loss, count = inside["loss"].view(torch.float64).reshape(()), inside["count"].view(torch.int64).reshape(())
    k.dn.grad(_dev(rows), _dev(target), grad, loss, count, 2.0 / B, _dev(nv), _dev(mask), value, extra, states_per_pass=1)
    torch.cuda.synchronize()
    for name, v in raw.items():
        b = v.cpu().numpy()
        assert (b[:pad] == CANARY).all() and (b[-pad:] == CANARY).all(), name
    assert_same((grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), extra.cpu().numpy().reshape(shape)),
                k.host(rows, target, nv, mask, 2.0 / B), "guarded")


@pytest.mark.parametrize("kind,ni", [("sarl", 1), ("lstm", 2)], ids=["sarl", "lstm"])
def test_more_chunks_than_one_launch_one_state_per_pass(kind, ni):
    k = kit(kind, ni)
    B = k.cases.chunk() * k.cases.max_chunks() + 9
    rows, target = k.cases.plain_batch(k.net, B, 2, seed=82)
    mask, nv = (np.arange(B) % 7 != 3).astype(np.uint8), (1 + np.arange(B) % 2).astype(np.int64)
    assert_same(k.kernel(rows, target, nv, mask, 2.0 / B, 1), k.host(rows, target, nv, mask, 2.0 / B), "two launches")


@pytest.mark.parametrize("kind,ni", [("sarl", 1), ("lstm", 2)], ids=["sarl", "lstm"])
def test_other_pass_sizes_are_invalid_and_a_capturing_stream_is_refused(kind, ni):
    k = kit(kind, ni)
    lib = _capi.lib()
    rows, target = k.cases.plain_batch(k.net, 3, 2, seed=83)
    want = k.host(rows, target, None, None, 1.0)
    entry = lib.ebc_sarl_net_grad_max_rows_at if kind == "sarl" else lib.ebc_lstm_net_grad_max_rows_at
    for bad in (3, 5, -1):
        grad, loss, count, value, extra = k.outputs(3, 2, poison=-5.0)
        with pytest.raises(_capi.EbcError) as err:
            k.dn.grad(_dev(rows), _dev(target), grad, loss, count, 1.0, None, None, value, extra, states_per_pass=bad)
        assert err.value.code == _abi.ERR_INVALID and "states_per_pass" in str(err.value)
        torch.cuda.synchronize()
        assert bool((grad == -5.0).all()) and float(loss) == -5.0 and int(count) == -5
        out = C.c_int(-9)
        assert entry(k.dn._h, bad, C.byref(out)) == _abi.ERR_INVALID and out.value == -9
    rd, td = _dev(rows), _dev(target)
    grad, loss, count, _, _ = k.outputs(3, 2, poison=-5.0)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        k.dn.grad(rd, td, grad, loss, count, 1.0, states_per_pass=1)  # scratch and the kernel's attributes are set before the capture
        side.synchronize()
        grad.fill_(-5.0)
        side.synchronize()
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError) as err:
                k.dn.grad(rd, td, grad, loss, count, 1.0, states_per_pass=1)
        finally:
            graph.capture_end()
        assert err.value.code == _abi.ERR_UNSUPPORTED and "captured" in str(err.value)
        side.synchronize()
        assert bool((grad == -5.0).all())
        k.dn.grad(rd, td, grad, loss, count, 1.0, states_per_pass=1)
        side.synchronize()
    assert sg.same_bytes(grad.cpu().numpy(), want[0]) and float(loss) == want[1] and int(count) == want[2]


# ------------------------------------------------------------------------------- 5. trainers
def _steps_against_float64(trainers, ref, xs, ys, sd, steps):
    """test_native_trainer_against_autograd_trainer's comparison and bar (tests/test_sarl_train_gpu.py): every step's loss
    and every tensor within TOL_FACTOR times torch's own float32 error (the larger of the CPU's and the device's) against
    the same steps in float64."""
    from test_sarl_train_gpu import _ratio
    (l64, w64), (l32c, w32c), (l32d, w32d) = ref["f64"], ref["f32_cpu"], ref["f32_dev"]
    n = int(ys.numel())
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


def test_sarl_trainer_auto_on_16_rows_against_the_autograd_trainer():
    """test_native_trainer_against_autograd_trainer at R = 16: 85 states of 16 rows, three SGD steps from the shipped a5
    weights, SarlTrainer(states_per_pass="auto") (two states per pass here) and SarlTrainer(native=False)."""
    import test_sarl_train_gpu as base
    from ebcsim.sarl_train import SarlTrainer
    sd, _, _, lr = base._golden_memory()
    states, values = sg.plain_batch(sg.REFERENCE_NET, 85, 16, seed=5016)
    ref = base._float64_steps(sd, states, values, lr, 3)
    trainers = {"auto": SarlTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=True, states_per_pass="auto"),
                "autograd": SarlTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=False, states_per_pass="auto")}
    assert trainers["auto"].passes.of(16) == 2 and trainers["auto"].grad_max_rows() == trainers["auto"].net.grad_max_rows(1)
    _steps_against_float64(trainers, ref, _dev(states), _dev(values), sd, 3)


def test_lstm_trainer_auto_on_16_rows_against_the_autograd_trainer():
    """The same for LstmTrainer on ValueNetwork2: 80 states of 16 rows, a seeded reference-width network."""
    import test_lstm_train_gpu as base
    from ebcsim.lstm_train import LstmTrainer
    sd, _, _, lr = base._memory(True)
    states, values = lg.plain_batch(lg.REFERENCE_NET2, 80, 16, seed=5017)
    ref = base._float64_steps(sd, states, values, lr, 3)
    trainers = {"auto": LstmTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=True, states_per_pass="auto"),
                "autograd": LstmTrainer(sd, device=DEV, optimizer="sgd", lr=lr, native=False, states_per_pass="auto")}
    assert trainers["auto"].passes.of(16) == 2
    _steps_against_float64(trainers, ref, _dev(states), _dev(values), sd, 3)


def test_auto_on_five_rows_is_the_default_trainer():
    """R = 5 fits the whole chunk: "auto" makes the default call, and three steps leave the default trainer's bytes."""
    import test_lstm_train_gpu as lbase
    import test_sarl_train_gpu as sbase
    from ebcsim.lstm_train import LstmTrainer
    from ebcsim.sarl_train import SarlTrainer
    for Trainer, (sd, states, values, lr) in ((SarlTrainer, sbase._golden_memory()), (LstmTrainer, lbase._memory(True))):
        a, b = Trainer(sd, device=DEV, lr=lr, states_per_pass="auto"), Trainer(sd, device=DEV, lr=lr)
        assert a.passes.of(5) == 0 and b.passes.of(5) == 0 and b.passes.of(99) == 0 and b.grad_max_rows() == b.net.grad_max_rows()
        xs, ys = _dev(states), _dev(values)
        for _ in range(3):
            for tr in (a, b):
                tr.loss_and_grad(xs, ys, grad_scale=2.0 / len(values))
                tr.step()
        assert torch.equal(a.flat.detach().view(torch.int32), b.flat.detach().view(torch.int32))


# ------------------------------------------------------------------------------- 6. the schedules end to end
def _sixteen_adults(policy_config, E=16):
    """E envs of sarl_a5.config with adult_num = 16 on device-generated train scenes with a restart pool.  16 adults barely
    fit that config's 4 m circle: the generator's rejection loops (one lane per scene, so fewer envs do not help) take 21 of
    the 22 s of each schedule test below on an MI355X; the schedule itself takes 0.7 s."""
    from ebcsim import actions as ebc_actions, config as ebc_config, scene as ebc_scene
    from ebcsim.batched import BatchedEnv
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"))
    cfg.set("sim", "adult_num", "16")
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", policy_config))
    params = ebc_config.params_from_config(cfg, pol)
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = ebc_scene.gen_struct(sc, "train")
    env = BatchedEnv(params, E, sum(gen.count), ebc_scene.max_static_rows(sc))
    env.use_torch_stream()
    seed0 = ebc_scene.COUNTER_OFFSET["train"]
    env.generate_reset(gen, seed0)
    env.generate_pool(gen, seed0 + E, 8 * E)
    return env, ebc_actions.build_action_space(sc.robot.v_pref)


SCHEDULE = dict(il_steps=40, il_epochs=2, train_iterations=3, steps_per_iteration=4, train_batches=4, batch_size=32, capacity=8192,
                epsilon_start=0.5, epsilon_end=0.5, target_update_interval=2)


def _schedule(run, make_trainer, reference_module, policy_config, tmp_path, entry):
    env, space = _sixteen_adults(policy_config)
    assert env.R == 16 and env.T == 13
    with pytest.raises(NotImplementedError, match="16 rows per state, %s takes" % entry):
        run(env, make_trainer(None), space, 0.9, generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path), **SCHEDULE)
    assert not list(tmp_path.iterdir())
    tr = make_trainer("auto")
    start = tr.state_dict()
    hist = run(env, tr, space, 0.9, generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path), **SCHEDULE)
    torch.cuda.synchronize()
    print(hist)
    assert hist["il_stored"] > 0 and hist["il_loss"] is not None and np.isfinite(hist["il_loss"])
    assert len(hist["rl_loss"]) == 3 and np.isfinite(hist["rl_loss"]).all() and np.isfinite(hist["mean_reward"]).all()
    assert hist["native_refreshes"] == 3
    for name in ("il_model.pth", "rl_model_3.pth"):
        loaded = torch.load(str(tmp_path / name), map_location="cpu")
        reference_module().load_state_dict(loaded, strict=True)
        assert all(bool(torch.isfinite(v).all()) for v in loaded.values())
    assert not all(torch.equal(loaded[k], start[k]) for k in start)
    env.close()


def test_sarl_schedule_on_sixteen_adults(tmp_path):
    """run_sarl_training on 16 envs of 16 adults, the shortest schedule of test_training_schedule_end_to_end, reference
    widths: the default trainer is refused as before, SarlTrainer(states_per_pass="auto") finishes with finite losses and
    its files load into SarlModule with strict=True."""
    from ebcsim.sarl_train import SarlTrainer, run_sarl_training

    def make(spp):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(11)
            return SarlTrainer(sg.module(sg.REFERENCE_NET), device=DEV, optimizer="sgd", lr=0.01, states_per_pass=spp)
    _schedule(run_sarl_training, make, lambda: sg.module(sg.REFERENCE_NET), "policy_plain.config", tmp_path, "ebc_sarl_grad")


def test_lstm_schedule_on_sixteen_adults(tmp_path):
    """The same for run_lstm_training with ValueNetwork2."""
    from ebcsim.lstm_train import LstmTrainer, run_lstm_training

    def make(spp):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(11)
            return LstmTrainer(lg.module(lg.REFERENCE_NET2), device=DEV, optimizer="sgd", lr=0.01, states_per_pass=spp)
    _schedule(run_lstm_training, make, lambda: lg.module(lg.REFERENCE_NET2), "policy_lstm.config", tmp_path, "ebc_lstm_grad")
