"""CADRL on the device: the decision kernel against the host build of the same rule (raw bytes) on every edge batch, its
independence of an env's place in the batch, its refusals, and the reference's golden runs through
DeviceSarlPolicy(CadrlValueNet).  Cases and tolerance: tests/cadrl_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from cadrl_cases import (ACTIONS, ENVS, ROWS, RUNS, TOL_FACTOR, all_edge_batches, chosen_index, edge_batch, golden_run,
                         golden_state_dict, host_decide, row_error)
from ebcsim import _abi, _capi
from helpers import Guarded, batch_from_init, params_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def decide(v, nv, reward, discount, values_ptr, choice_ptr, E=None, A=None, R=None, check=True):
    """One ebc_cadrl_decide on the current stream: v, nv (or None), reward are device tensors."""
    a = _abi.EbcCadrlArgs()
    a.struct_size = C.sizeof(a)
    shape = tuple(v.shape) if v.dim() == 3 else (None, None, None)
    a.E, a.A, a.R = [int(s if o is None else o) for s, o in zip(shape, (E, A, R))]
    a.discount = float(discount)
    a.v, a.reward, a.values, a.choice = v.data_ptr(), reward.data_ptr(), values_ptr, choice_ptr
    a.n_valid = None if nv is None else nv.data_ptr()
    rc = _capi.lib().ebc_cadrl_decide(torch.cuda.current_stream().cuda_stream, C.addressof(a))
    if check:
        _capi.check(rc)
    return rc


def kernel_decide(v, nv, reward, discount):
    """(values, choice) of the kernel on host arrays, its outputs between canaries and every element of them written."""
    E, A, R = v.shape
    vd, rd = torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(reward)).to(DEV)
    nd = None if nv is None else torch.from_numpy(np.ascontiguousarray(nv)).to(DEV)
    gv, gc = Guarded((E, A), torch.float64, device=DEV), Guarded((E,), torch.int32, device=DEV)
    decide(vd, nd, rd, discount, gv.ptr, gc.ptr)
    torch.cuda.synchronize()
    return gv.check(), gc.check()


@pytest.mark.parametrize("A", ACTIONS)
def test_kernel_equals_host_build_bytes(A):
    """Every edge batch of this action count (E in 1, 3, 65; R in 1, 2, 18, 33; ragged n_valid with 0, 1, R, values above R
    and below 0; NaN in valid rows; NaN and both infinities in padding rows; all-NaN envs; exact ties across and inside the
    lane halves; infinities as values): values and choice are the host build's, byte for byte, and nothing outside the
    two outputs is written."""
    for E in ENVS:
        for R in ROWS:
            v, nv, reward, discount, kinds = all_edge_batches()[E, A, R]
            want_values, want_choice = host_decide(v, nv, reward, discount)
            values, choice = kernel_decide(v, nv, reward, discount)
            tag = "E %d A %d R %d" % (E, A, R)
            assert values.tobytes() == want_values.tobytes(), (tag, np.argwhere(values.view(np.int64) != want_values.view(np.int64))[:3].tolist())
            assert choice.tobytes() == want_choice.tobytes(), (tag, choice.tolist(), want_choice.tolist())
            for e, kind in enumerate(kinds):
                if kind in ("all_nan", "no_rows"):
                    assert choice[e] == -1, (tag, e, kind)
    # n_valid = NULL: all R rows
    v, nv, reward, discount, _ = all_edge_batches()[65, A, 18]
    want = host_decide(v, None, reward, discount)
    got = kernel_decide(v, None, reward, discount)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_env_result_does_not_depend_on_its_place():
    """One env at indices 0, 1, 31, 64 and last among envs of other row counts and kinds: the same bytes, the host build's."""
    A, R, E = 81, 18, 67
    v, nv, reward, discount, _ = edge_batch(E, A, R, seed=77)
    rs = np.random.RandomState(78)
    pv, pn, pr = rs.normal(0.0, 1.5, (1, A, R)).astype(np.float32), np.array([11], dtype=np.int64), np.round(rs.normal(0.0, 0.3, (1, A)), 2)
    pv[0, :, 11:] = np.nan
    pv[0, 7] = pv[0, 71]
    pr[0, 7] = pr[0, 71] = 2.0  # the best value twice, 64 actions apart
    pv[0, [7, 71], :11] += np.float32(40.0)
    want_values, want_choice = host_decide(pv, pn, pr, discount)
    assert want_choice[0] == 7
    for at in (0, 1, 31, 64, E - 1):
        v2, n2, r2 = v.copy(), nv.copy(), reward.copy()
        v2[at], n2[at], r2[at] = pv[0], pn[0], pr[0]
        values, choice = kernel_decide(v2, n2, r2, discount)
        assert values[at].tobytes() == want_values[0].tobytes() and choice[at] == 7, at


def test_refusals_and_capture():
    """A = 129 and R = 129 are refused by name before anything is launched; a decision on a stream under capture is
    refused with EBC_ERR_UNSUPPORTED and the entry stays usable."""
    lib = _capi.lib()
    v, nv, reward, discount, _ = all_edge_batches()[3, 81, 18]
    want_values, want_choice = host_decide(v, nv, reward, discount)
    vd, nd, rd = torch.from_numpy(v).to(DEV), torch.from_numpy(nv).to(DEV), torch.from_numpy(reward).to(DEV)
    values = torch.full((3, 81), -5.0, dtype=torch.float64, device=DEV)
    choice = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    big = torch.zeros((129 * 129,), dtype=torch.float32, device=DEV)
    big_r = torch.zeros((129,), dtype=torch.float64, device=DEV)
    big_out = torch.zeros((129,), dtype=torch.float64, device=DEV)
    assert decide(big, None, big_r, discount, big_out.data_ptr(), choice.data_ptr(), E=1, A=129, R=1, check=False) == _abi.ERR_UNSUPPORTED
    assert b"A > 128" in lib.ebc_last_error()
    assert decide(big, None, big_r, discount, big_out.data_ptr(), choice.data_ptr(), E=1, A=1, R=129, check=False) == _abi.ERR_UNSUPPORTED
    assert b"R > 128" in lib.ebc_last_error()
    torch.cuda.synchronize()
    assert (values == -5.0).all() and (choice == -5).all() and (big_out == 0).all()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        decide(vd, nd, rd, discount, values.data_ptr(), choice.data_ptr())
        side.synchronize()
        graph.capture_begin()
        try:
            rc = decide(vd, nd, rd, discount, values.data_ptr(), choice.data_ptr(), check=False)
        finally:
            graph.capture_end()
        assert rc == _abi.ERR_UNSUPPORTED and b"captured" in lib.ebc_last_error()
        values.fill_(-5.0)
        decide(vd, nd, rd, discount, values.data_ptr(), choice.data_ptr())
        side.synchronize()
    assert values.cpu().numpy().tobytes() == want_values.tobytes() and choice.cpu().numpy().tobytes() == want_choice.tobytes()


def test_value_net_refuses_networks_the_blocks_do_not_take():
    """Three layers, or two outputs: NotImplementedError on the device, never a torch path."""
    from ebcsim.cadrl import CadrlModule, CadrlValueNet
    rows = torch.zeros((2, 3, 13), dtype=torch.float32, device=DEV)
    for dims in ([150, 100, 1], [150, 100, 100, 2]):
        net = CadrlValueNet(CadrlModule(13, dims).state_dict(), device=DEV)
        with pytest.raises(NotImplementedError):
            net.forward(rows)
        assert net.native_forwards == 0


def test_forward_is_the_minimum_over_the_rows_that_exist():
    """CadrlValueNet.forward on the device: the torch module's minimum over each state's own rows within TOL_FACTOR * e_ref,
    NaN for a state without rows, padding rows (NaN) never entering.  (A NaN the NETWORK gives in a valid row is the
    kernel's to propagate and is held to the host build above; what the float32 blocks make of a NaN input is theirs.)"""
    from ebcsim.cadrl import CadrlValueNet
    _, meta, m32, m64 = golden_run("cadrl_a5")
    rows = torch.randn(70, 5, 13, generator=torch.Generator().manual_seed(9))
    nv = torch.randint(0, 6, (70,), generator=torch.Generator().manual_seed(10))
    nv[0], nv[1], nv[2] = 0, 5, 3
    rows[torch.arange(5)[None, :] >= nv[:, None]] = float("nan")
    net = CadrlValueNet(golden_state_dict(meta), device=DEV)
    got = net.forward(rows.to(DEV), nv.to(DEV)).cpu()
    with torch.no_grad():
        want = m32(torch.nan_to_num(rows, nan=0.0), nv)
    assert got.dtype == torch.float32 and net.native_forwards == 1
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(got[0]) and not torch.isnan(got[1:3]).any()
    tol = TOL_FACTOR * row_error(m32, m64, torch.nan_to_num(rows, nan=0.0))
    assert float(torch.nan_to_num(got - want, nan=0.0).abs().max()) <= tol
    full = net.forward(rows[nv == 5].to(DEV)).cpu()
    assert torch.equal(full, got[nv == 5])


@pytest.mark.parametrize("name", RUNS)
def test_cadrl_decisions_gpu(name):
    """The golden run on five copies, DeviceSarlPolicy(CadrlValueNet) deciding: every recorded value within
    TOL_FACTOR * e_ref, all copies agreeing, the recorded action at EVERY decision (by the policy's argmax and by the
    kernel's own choice), the recorded infos and rewards; every forward native.  The last decisions run through
    DeviceCadrlPolicy, which takes the kernel's choice."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.cadrl import CadrlValueNet, DeviceCadrlPolicy
    from ebcsim.sarl import DeviceSarlPolicy
    z, meta, m32, m64 = golden_run(name)
    params = params_of(z)
    E = 5
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params, E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = CadrlValueNet(golden_state_dict(meta), device=DEV)
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"])
    own = DeviceCadrlPolicy(net, z["action_space"], meta["gamma"])
    outs = env.alloc_step_outputs(("reward", "done", "info"))
    T = len(z["action"])
    e_ref, errs = 0.0, []
    for t in range(T):
        use = own if t >= T - 10 else pol
        actions, values = use.decide(env)
        torch.cuda.synchronize()
        v = values.cpu().numpy()
        assert (v == v[0:1]).all(), "the copies disagree at decision %d" % t
        e_ref = max(e_ref, row_error(m32, m64, use._bufs["rows_rotated"][0]))
        errs.append(float(np.abs(v[0] - z["values"][t]).max()))
        want = chosen_index(z, t)
        assert net.last_choice.cpu().tolist() == [want] * E, t
        np.testing.assert_array_equal(actions.cpu().numpy(), np.tile(z["action"][t], (E, 1)), err_msg="decision %d" % t)
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_CACHED)
        torch.cuda.synchronize()
        assert int(outs["info"][0]) == int(z["info"][t]), t
        np.testing.assert_allclose(float(outs["reward"][0]), z["reward"][t], atol=1e-9)
    tol = TOL_FACTOR * e_ref
    print("%s: %d decisions, e_ref %.3g, tolerance %.3g, |values - recorded| %.3g" % (name, T, e_ref, tol, max(errs)))
    assert max(errs) <= tol, (max(errs), tol)
    assert int(z["info"][-1]) == int(meta["final_info"])
    assert net._native_blocks() is not None and net.native_forwards >= T > 0
