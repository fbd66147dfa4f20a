"""SAIL on the device: the fused network kernel against the host build of the same arithmetic (raw bytes, action and
feat_joint) on every edge batch, its independence of an env's place in the batch, its refusals, the reference's golden run
through SailNet on the device, and DeviceSailPolicy on a BatchedEnv.  Cases and tolerance: tests/sail_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from sail_cases import (ADULTS, TOL_FACTOR, check_kinds, edge_batch, env_counts, golden, host_forward, host_group, layer_arrays,
                        random_state_dict, ref_error, same_bytes)
from ebcsim import _abi, _capi
from helpers import Guarded, batch_from_init, params_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_nets = {}


def net_of(N, scale):
    from ebcsim.sail import SailNet
    if (N, scale) not in _nets:
        _nets[N, scale] = SailNet(random_state_dict(N, scale), device=DEV)
    return _nets[N, scale]


def forward(handle, robot, ob, n_rows, action_ptr, feat_ptr, E=None, R=None, check=True):
    """One ebc_sail_forward on the current stream: robot, ob, n_rows (or None) are device tensors."""
    a = _abi.EbcSailArgs()
    a.struct_size = C.sizeof(a)
    a.E, a.R = int(ob.shape[0] if E is None else E), int(ob.shape[1] if R is None else R)
    a.robot, a.ob, a.action, a.feat_joint = robot.data_ptr(), ob.data_ptr(), action_ptr, feat_ptr
    a.n_rows = None if n_rows is None else n_rows.data_ptr()
    rc = _capi.lib().ebc_sail_forward(handle, torch.cuda.current_stream().cuda_stream, C.addressof(a))
    if check:
        _capi.check(rc)
    return rc


def kernel_forward(net, robot, ob, n_rows, want_feat=True):
    """(action, feat_joint or None) of the kernel on host arrays, its outputs between canaries and every element written."""
    E = ob.shape[0]
    rd, od = torch.from_numpy(np.ascontiguousarray(robot)).to(DEV), torch.from_numpy(np.ascontiguousarray(ob)).to(DEV)
    nd = None if n_rows is None else torch.from_numpy(np.ascontiguousarray(n_rows)).to(DEV)
    ga = Guarded((E, 2), torch.float64, device=DEV)
    gf = Guarded((E, 64), torch.float32, device=DEV) if want_feat else None
    forward(net.native()._h, rd, od, nd, ga.ptr, gf.ptr if want_feat else None)
    torch.cuda.synchronize()
    return ga.check(), gf.check() if want_feat else None


@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("N", ADULTS)
def test_kernel_equals_host_build_bytes(N, scale):
    """Every edge batch of this adult_num and weight scale (E in 1, G - 1, G, G + 1, 2 G + 1, 7 and one whose last tile is
    short; R = N and N + 3; NaN and infinities in the padding rows; ragged row counts; arrived envs; a NaN inside a valid
    row; equal logits; zero velocities): action and feat_joint are the host build's, byte for byte, nothing outside the
    two outputs is written and every element of them is; feat_joint = NULL and n_rows = NULL work."""
    from ebcsim.sail import envs_per_workgroup
    net, sd = net_of(N, scale), random_state_dict(N, scale)
    assert host_group(N) == envs_per_workgroup(N)
    for R in (N, N + 3):
        for E in env_counts(N):
            robot, ob, n_rows, kinds = edge_batch(N, E, R)
            want = host_forward(sd, robot, ob, n_rows)
            action, feat = kernel_forward(net, robot, ob, n_rows)
            tag = "N %d E %d R %d x%d" % (N, E, R, scale)
            assert same_bytes(action, want[0]), (tag, np.argwhere(action.view(np.int64) != want[0].view(np.int64))[:3].tolist())
            assert same_bytes(feat, want[1]), (tag, np.argwhere(feat.view(np.int32) != want[1].view(np.int32))[:3].tolist())
            check_kinds(action, feat, n_rows, kinds, N, tag)
    E = env_counts(N)[-1]
    robot, ob, n_rows, _ = edge_batch(N, E, N + 3)
    want = host_forward(sd, robot, ob, None)
    action, feat = kernel_forward(net, robot, ob, None)
    assert same_bytes(action, want[0]) and same_bytes(feat, want[1])
    action, none = kernel_forward(net, robot, ob, n_rows, want_feat=False)
    assert none is None and same_bytes(action, host_forward(sd, robot, ob, n_rows)[0])
    assert net.native_forwards == 0  # the entry itself was called; SailNet.forward is tested below


def test_env_result_does_not_depend_on_its_place():
    """One env at indices 0, 1, G and last among envs of every kind: the same bytes, the host build's."""
    N = 5
    G = host_group(N)
    E = 2 * G + 3
    net, sd = net_of(N, 8), random_state_dict(N, 8)
    robot, ob, n_rows, _ = edge_batch(N, E, N + 3, seed=77)
    pr, po, pn, _ = edge_batch(N, 1, N + 3, seed=78)
    pn[0] = N
    want = host_forward(sd, pr, po, pn)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for at in (0, 1, G, E - 1):
        r2, o2, n2 = robot.copy(), ob.copy(), n_rows.copy()
        r2[at], o2[at], n2[at] = pr[0], po[0], pn[0]
        action, feat = kernel_forward(net, r2, o2, n2)
        assert same_bytes(action[at], want[0][0]) and same_bytes(feat[at], want[1][0]), at


def test_refusals_and_capture():
    """adult_num 1 and 33 are refused by name, R < adult_num is refused before anything is launched, and a forward on a
    stream under capture is refused with EBC_ERR_UNSUPPORTED and leaves the entry usable."""
    lib = _capi.lib()
    N = 5
    net, sd = net_of(N, 1), random_state_dict(N, 1)
    w, b = layer_arrays(random_state_dict(2))
    for n, text in ((1, b"adult_num < 2"), (33, b"adult_num > 32")):
        s = _abi.EbcSailWeights()
        s.struct_size, s.adult_num = C.sizeof(s), n
        for i in range(_abi.SAIL_LAYERS):
            s.weight[i], s.bias[i] = w[i].ctypes.data, b[i].ctypes.data
        h = C.c_void_p()
        assert lib.ebc_sail_create(C.addressof(s), 0, C.byref(h)) == _abi.ERR_UNSUPPORTED and text in lib.ebc_last_error()
        assert not h
    robot, ob, n_rows, _ = edge_batch(N, 9, N + 3)
    want = host_forward(sd, robot, ob, n_rows)
    rd, od, nd = torch.from_numpy(robot).to(DEV), torch.from_numpy(ob).to(DEV), torch.from_numpy(n_rows).to(DEV)
    action = torch.full((9, 2), -5.0, dtype=torch.float64, device=DEV)
    feat = torch.full((9, 64), -5.0, dtype=torch.float32, device=DEV)
    h = net.native()._h
    assert forward(h, rd, od, nd, action.data_ptr(), feat.data_ptr(), R=N - 1, check=False) == _abi.ERR_INVALID
    assert b"R < adult_num" in lib.ebc_last_error()
    torch.cuda.synchronize()
    assert (action == -5.0).all() and (feat == -5.0).all()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        forward(h, rd, od, nd, action.data_ptr(), feat.data_ptr())
        side.synchronize()
        graph.capture_begin()
        try:
            rc = forward(h, rd, od, nd, action.data_ptr(), feat.data_ptr(), check=False)
        finally:
            graph.capture_end()
        assert rc == _abi.ERR_UNSUPPORTED and b"captured" in lib.ebc_last_error()
        action.fill_(-5.0)
        forward(h, rd, od, nd, action.data_ptr(), feat.data_ptr())
        side.synchronize()
    assert same_bytes(action.cpu().numpy(), want[0]) and same_bytes(feat.cpu().numpy(), want[1])


@pytest.mark.parametrize("name", ["sail_a5", "sail_cases"])
def test_recorded_outputs_on_the_device(name):
    """The recorded states through SailNet on the device: every recorded action and feat_joint within TOL_FACTOR * e_ref,
    and the host build's bytes."""
    from ebcsim.sail import SailNet
    z, meta, sd, m32, m64 = golden(name)
    robot, ob = z["robot"], z["ob"]
    decided = z["decided"].astype(bool) if "decided" in z.files else np.ones(len(robot), dtype=bool)
    e_ref = ref_error(m32, m64, robot, ob)
    net = SailNet(sd, device=DEV)
    action, feat = net.forward(torch.from_numpy(robot).to(DEV), torch.from_numpy(ob).to(DEV))
    action, feat = action.cpu().numpy(), feat.cpu().numpy()
    assert net.native_forwards == 1 and action.dtype == np.float64 and feat.dtype == np.float32
    want = host_forward(sd, robot, ob)
    assert same_bytes(action, want[0]) and same_bytes(feat, want[1])
    errs = float(np.abs(action - z["action"]).max()), float(np.abs(feat[decided] - z["feat_joint"][decided]).max())
    print("%s: e_ref %.3g / %.3g, |device - recorded| %.3g / %.3g (action / feat_joint)" % ((name,) + e_ref + errs))
    assert errs[0] <= TOL_FACTOR * e_ref[0] and errs[1] <= TOL_FACTOR * e_ref[1], (errs, e_ref)
    assert (action[~decided] == 0).all()


def test_device_policy_on_the_golden_scene_and_twenty_steps():
    """DeviceSailPolicy.decide on a BatchedEnv reset to the golden scene (five copies) gives the first recorded action
    within the bound on every copy, from device buffers alone; then the batch steps 20 times under the policy without a
    NaN in any action, every decision one native forward."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy, SailNet
    z, meta, sd, m32, m64 = golden("sail_a5")
    tol = TOL_FACTOR * ref_error(m32, m64, z["robot"], z["ob"])[0]
    E = 5
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params_of(z), E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = SailNet(sd, device=DEV)
    pol = DeviceSailPolicy(net)
    actions, values = pol.decide(env)
    torch.cuda.synchronize()
    assert values is None and actions.is_cuda and actions.dtype == torch.float64 and tuple(actions.shape) == (E, 2)
    got = actions.cpu().numpy()
    assert (got == got[0:1]).all() and np.abs(got[0] - z["action"][0]).max() <= tol, (got[0], z["action"][0])
    np.testing.assert_allclose(pol._bufs["robot"].cpu().numpy()[0], z["robot"][0], atol=1e-12)
    np.testing.assert_allclose(pol._bufs["ob"].cpu().numpy()[0, :5], z["ob"][0], atol=1e-12)
    assert pol._bufs["n_rows"].cpu().tolist() == [5] * E
    outs = env.alloc_step_outputs(("reward", "done", "info"))
    for t in range(20):
        actions, _ = pol.decide(env)
        assert bool(torch.isfinite(actions).all()), t
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_ORCA)
    torch.cuda.synchronize()
    assert net.native_forwards == 21
    env.close()
