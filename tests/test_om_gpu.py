"""OM-SARL on the device: ebc_occupancy_rows against the host build of the same rule (raw bytes, both outputs between
canaries) at every shape of the sweep, each output alone, its refusals, and the reference's recorded OM-SARL runs through
DeviceSarlPolicy(om=spec).  Cases and tolerances: tests/om_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi
from ebcsim.occupancy import OccupancySpec, occupancy_rows_device
from helpers import GOLDEN, Guarded, batch_from_init, load, params_of
from om_cases import GRIDS, REFUSALS, RUNS, chosen_index, edge_batch, golden_run, golden_state_dict, host_om, om_args, shape_sweep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5  # the bar tests/test_sarl.py holds the recorded values of the non-OM goldens to


def kernel_om(ob, nv, spec, rows=None, want_om=True):
    """(om, rows_wide) of the kernel on host arrays, each output between canaries and every element of it written."""
    E, R = ob.shape[:2]
    obd = torch.from_numpy(np.ascontiguousarray(ob)).to(DEV)
    nd = None if nv is None else torch.from_numpy(np.ascontiguousarray(nv)).to(DEV)
    g_om = Guarded((E, R, spec.width), torch.float32, device=DEV) if want_om else None
    rd = g_wide = None
    if rows is not None:
        rd = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
        g_wide = Guarded(rows.shape[:3] + (rows.shape[3] + spec.width,), torch.float32, device=DEV)
    occupancy_rows_device(obd, nd, spec, rows=rd, om_out=None if g_om is None else g_om.t,
                          wide_out=None if g_wide is None else g_wide.t, want_om=want_om)
    torch.cuda.synchronize()
    return (None if g_om is None else g_om.check()), (None if g_wide is None else g_wide.check())


@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_kernel_equals_host_build_bytes(grid):
    """Every shape of this grid's sweep (E in 1, 3, 65; R in 1, 2, 18, 33, 128; A in 1, 2, 81; T in 13, 17; ragged n_valid with
    0, 1, R, values above R and below 0; NaN in every row past n_valid; occupants far outside the grid; coincident rows;
    zero velocities of both signs): om and rows_wide are the host build's, byte for byte, every element written and
    nothing outside the two outputs; then om alone, rows_wide alone, and n_valid = NULL."""
    cell_num, channels = GRIDS[grid]
    seen_a, seen_t = set(), set()
    for E, R, A, T in shape_sweep(grid):
        ob, nv, rows, spec = edge_batch(E, R, A, T, cell_num, channels)
        want_om, want_wide = host_om(ob, nv, spec, rows)
        om, wide = kernel_om(ob, nv, spec, rows)
        tag = "E %d R %d A %d T %d grid %s" % (E, R, A, T, GRIDS[grid])
        assert om.tobytes() == want_om.tobytes(), (tag, np.argwhere(om.view(np.uint32) != want_om.view(np.uint32))[:3].tolist())
        assert wide.tobytes() == want_wide.tobytes(), (tag, np.argwhere(wide.view(np.uint32) != want_wide.view(np.uint32))[:3].tolist())
        assert np.isfinite(om).all(), tag
        seen_a.add(A)
        seen_t.add(T)
    assert seen_a == {1, 2, 81} and seen_t == {13, 17}
    E, R, A, T = 3, 18, 81, 17
    ob, nv, rows, spec = edge_batch(E, R, A, T, cell_num, channels)
    want_om, want_wide = host_om(ob, nv, spec, rows)
    om, none = kernel_om(ob, nv, spec)
    assert none is None and om.tobytes() == want_om.tobytes()
    none, wide = kernel_om(ob, nv, spec, rows, want_om=False)
    assert none is None and wide.tobytes() == want_wide.tobytes()
    clean = np.nan_to_num(ob, nan=0.25)
    want = host_om(clean, None, spec, rows)
    got = kernel_om(clean, None, spec, rows)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_refusals_and_capture():
    """Every refusal of the entry with device buffers behind the pointers, nothing written; a stream under capture is refused
    with EBC_ERR_UNSUPPORTED and the entry stays usable."""
    lib = _capi.lib()
    ob, nv, rows, spec = edge_batch(3, 18, 2, 13, 4, 3)
    want_om, want_wide = host_om(ob, nv, spec, rows)
    obd, nd, rd = (torch.from_numpy(x).to(DEV) for x in (ob, nv, rows))
    big = torch.full((1 << 20,), -5.0, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for kw, reason in REFUSALS:
        kw = dict(kw)
        ptrs = dict(next_ob=obd.data_ptr(), rows=rd.data_ptr(), om=big.data_ptr(), rows_wide=big.data_ptr())
        ptrs.update({k: kw.pop(k) for k in list(kw) if k in ptrs})
        a = om_args(**dict(dict(E=1, R=2, A=1, T=13), **kw), **ptrs)
        assert lib.ebc_occupancy_rows(0, stream, C.addressof(a)) == _abi.ERR_UNSUPPORTED, (kw, reason)
        assert reason in lib.ebc_last_error(), (reason, lib.ebc_last_error())
    torch.cuda.synchronize()
    assert (big == -5.0).all()
    om = torch.full((3, 18, spec.width), -5.0, dtype=torch.float32, device=DEV)
    wide = torch.full((3, 2, 18, 13 + spec.width), -5.0, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        occupancy_rows_device(obd, nd, spec, rows=rd, om_out=om, wide_out=wide)
        side.synchronize()
        om.fill_(-5.0)
        graph.capture_begin()
        try:
            with pytest.raises(_capi.EbcError) as err:
                occupancy_rows_device(obd, nd, spec, rows=rd, om_out=om, wide_out=wide)
        finally:
            graph.capture_end()
        assert err.value.code == _abi.ERR_UNSUPPORTED and b"captured" in lib.ebc_last_error()
        side.synchronize()
        assert (om == -5.0).all()
        occupancy_rows_device(obd, nd, spec, rows=rd, om_out=om, wide_out=wide)
        side.synchronize()
    assert om.cpu().numpy().tobytes() == want_om.tobytes() and wide.cpu().numpy().tobytes() == want_wide.tobytes()


@pytest.mark.parametrize("name", RUNS)
def test_om_sarl_decisions_gpu(name):
    """The recorded run on five copies, DeviceSarlPolicy(om=spec) deciding: the reference's action at EVERY decision, every
    recorded value within TOL, the recorded infos and rewards; mlp1 of width T + W ran in the library (matrix-core and
    float32 forms, no torch GEMM), and the refinement's bound was never violated."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    z, meta, spec, _, _ = golden_run(name)
    params = params_of(z)
    E = 5
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params, E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = SarlValueNet(golden_state_dict(meta), device=DEV, with_global_state=meta["with_global_state"])
    assert net.input_dim == env.T + spec.width == meta["input_dim"]
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"], om=spec)
    outs = env.alloc_step_outputs(("reward", "done", "info"))
    steps = len(z["action"])
    errs = []
    for t in range(steps):
        actions, values = pol.decide(env)
        torch.cuda.synchronize()
        v = values.cpu().numpy()
        assert (np.abs(v - v[0:1]) < 1e-5).all(), "the copies disagree at decision %d" % t
        errs.append(float(np.abs(v[0] - z["values"][t]).max()))
        assert int(np.argmax(v[0])) == chosen_index(z, t), "decision %d" % t
        np.testing.assert_array_equal(actions.cpu().numpy(), np.tile(z["action"][t], (E, 1)), err_msg="decision %d" % t)
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_CACHED)
        torch.cuda.synchronize()
        assert int(outs["info"][0]) == int(z["info"][t]), t
        np.testing.assert_allclose(float(outs["reward"][0]), z["reward"][t], atol=1e-9)
    print("%s: %d decisions, |values - recorded| %.3g (bar %.3g), forwards %d matrix-core / %d float32 / %d float32 mlp1 only, "
          "refine stats %s" % (name, steps, max(errs), TOL, getattr(net, "native_forwards", 0), getattr(net, "native_exact_forwards", 0),
                               getattr(net, "native_exact_mlp1_forwards", 0), net.refine_stats))
    assert max(errs) <= TOL, max(errs)
    assert int(z["info"][-1]) == int(meta["final_info"])
    blocks = net._native_blocks()
    assert blocks is not None and blocks[0].K0 == env.T + spec.width, "mlp1 of width T + W is not a library block"
    assert getattr(net, "native_forwards", 0) >= steps > 0
    assert net.refine_stats["bound_violations"] == 0, net.refine_stats
    if net.refine_stats["candidates"]:
        # the whole float32 form in the library, or (a network whose mlp2 has 50 outputs: the pair kernels do not take it)
        # at least mlp1, the stack that sees the wide rows
        assert getattr(net, "native_exact_forwards", 0) + getattr(net, "native_exact_mlp1_forwards", 0) > 0, \
            "the float32 form of mlp1 did not run in the library"
    # the maps on the device are the host rule's on the last sweep's rows
    ob = pol._bufs["next_ob"].cpu().numpy()
    assert pol._wide[..., env.T:].cpu().numpy()[:, 0].tobytes() == host_om(ob, None, spec)[0].tobytes()


def test_policy_without_maps_is_unchanged():
    """DeviceSarlPolicy(om=None) on an existing golden episode: byte-identical values to a policy built without the
    argument, and a network of the wrong width for the maps is a ValueError."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    z = load("sarl_a5_baseline")
    meta = json.loads(str(z["meta"]))
    params = params_of(z)
    E = 5
    b = batch_from_init(z, copies=E)
    got = []
    for kw in ({}, {"om": None}):
        env = BatchedEnv(params, E, b.N, b.S)
        env.reset(b)
        env.use_torch_stream()
        net = SarlValueNet.load(os.path.join(GOLDEN, "weights", meta["weights"]), device=DEV)
        pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"], **kw)
        outs = env.alloc_step_outputs(("reward", "done", "info"))
        vals = []
        for t in range(12):
            _, values = pol.decide(env)
            vals.append(values.cpu().numpy().copy())
            forced = torch.tensor(np.tile(z["action"][t], (E, 1)), dtype=torch.float64, device=DEV)
            env.step_device(outs, robot_action=forced, human_policy=_abi.HUMAN_CACHED)
        torch.cuda.synchronize()
        assert "next_ob" not in pol._bufs and not hasattr(pol, "_wide")
        got.append(np.stack(vals))
    assert got[0].tobytes() == got[1].tobytes()
    ok = ~np.isnan(z["values"][:12]).any(1)
    assert ok.any()
    np.testing.assert_allclose(got[0][ok, 0], z["values"][:12][ok], atol=TOL, rtol=0)
    with pytest.raises(ValueError, match="wide"):
        DeviceSarlPolicy(net, z["action_space"], meta["gamma"], om=OccupancySpec(4, 1.0, 3)).decide(env)
