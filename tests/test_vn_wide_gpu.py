"""The wide two-layer value-network block (ebc_mlp2_create_wide: K0, H, O up to 640; csrc/ebc_vn_wide.h) and the networks
that decide with it (SarlValueNet(..., wide=True)) on the device: the coarse (split-bf16) form and the float32 form against
float64, the attention form, the wide entry against the narrow block at shapes both take, the device-side re-pack, the
refusals, whole x3 / x4 networks, decisions against the torch path, and the training schedule with wide_decide.  Every
buffer a kernel writes is a helpers.Guarded one.  Cases: tests/vn_wide_cases.py; weights, inputs and float64 references:
tests/value_net_cases.py (make_block / mlp2_ref, the recipe of tests/test_value_net.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import value_net_cases as vc
import vn_wide_cases as wc
from helpers import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_blocks = {}


def _block(shape, tail=False, wide=True, seed=None):
    """(weights, Mlp2Block) of a seeded block, made once per (shape, tail, entry)."""
    key = (shape, tail, wide, seed)
    if key not in _blocks:
        from ebcsim.mlp2 import Mlp2Block
        w, _ = vc.make_block(*shape, tail=tail, seed=seed)
        t = torch.from_numpy
        fin = (t(w["w3"]).reshape(1, -1), t(w["b3"])) if tail else None
        _blocks[key] = (w, Mlp2Block([(t(w["w1"]), t(w["b1"])), (t(w["w2"]), t(w["b2"]))], 0, final=fin, wide=wide))
    return _blocks[key]


def _y(blk, M):
    return Guarded((M,) if blk.has_final else (M, blk.O), torch.float32)


def _run(entry, x, relu_out, row_bias=None, group_rows=0, blk=None):
    """One forward into a guarded buffer -> its checked contents."""
    y = _y(blk, x.shape[0])
    entry(x, relu_out, row_bias=row_bias, group_rows=group_rows, out=y.t)
    torch.cuda.synchronize()
    return y.check()


def _inputs(shape, M, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(M, shape[0]) * 2).astype(np.float32)


# ---- 1. the coarse block against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu_out", [0, 1])
@pytest.mark.parametrize("shape", wc.BLOCK_SHAPES, ids=["x".join(map(str, s)) for s in wc.BLOCK_SHAPES])
def test_coarse_block_against_float64(shape, relu_out):
    """err <= 4e-5 * max(scale, 1), the bar of test_mlp2_split_bf16_matches_float32 (a CPU emulation of the split stays at
    or below 0.20 of it at the first nine shapes), at row counts with a part-filled last tile, and at 400 x 400 x 200 with
    waves and workgroups past the last row tile; two calls give the same bytes."""
    w, blk = _block(shape)
    counts = wc.ROW_COUNTS + (wc.EDGE_ROW_COUNTS if shape == wc.EDGE_SHAPE else ())
    x = _inputs(shape, max(counts), shape[0] * 7 + shape[1])
    ref = vc.mlp2_ref(x, w, relu_out)
    xd = torch.from_numpy(x).cuda()
    for M in counts:
        got = _run(blk, xd[:M], relu_out, blk=blk)
        err, scale = float(np.abs(got - ref[:M]).max()), float(np.abs(ref[:M]).max())
        print("coarse %s relu %d M %d: error %.3g, scale %.3g, bar %.3g" % (shape, relu_out, M, err, scale, 4e-5 * max(scale, 1.0)))
        assert err <= 4e-5 * max(scale, 1.0), (shape, relu_out, M, err, scale)
        assert np.array_equal(got.view(np.uint32), _run(blk, xd[:M], relu_out, blk=blk).view(np.uint32)), (shape, M)


# ---- 2. the attention form: group term + one-output tail ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,R,B", wc.ATTENTION_CASES, ids=["%s_R%d" % ("x".join(map(str, c[0])), c[1]) for c in wc.ATTENTION_CASES])
def test_attention_form(shape, R, B):
    """The per-group term on the hidden pre-activation (H up to 640) and the tail's dot product across the output passes,
    coarse and float32; once more with a last group that is partial (the last pair loses three rows, or the only row of
    its neighbour)."""
    w, blk = _block(shape, tail=True)
    rs = np.random.RandomState(shape[0] + R)
    x = _inputs(shape, B * R, shape[0] + 31 * R)
    g = rs.randn(B, shape[1]).astype(np.float32)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    for M in (B * R, B * R - min(3, R)):
        assert M % 32 != 0 or M != B * R
        groups = -(-M // R)
        ref = vc.mlp2_ref(x[:M], w, 0, g[:groups], R)
        bar = 4e-5 * max(float(np.abs(ref).max()), 1.0)
        got = _run(blk, xd[:M], 0, gd[:groups], R, blk=blk)
        err = float(np.abs(got - ref).max())
        print("attention %s R %d M %d: coarse error %.3g, bar %.3g" % (shape, R, M, err, bar))
        assert err <= bar, (shape, R, M, err)
        assert np.array_equal(got.view(np.uint32), _run(blk, xd[:M], 0, gd[:groups], R, blk=blk).view(np.uint32))
        f32 = _run(blk.f32, xd[:M], 0, gd[:groups], R, blk=blk)
        assert float(np.abs(f32 - ref).max()) <= bar, (shape, R, M)


# ---- 3. the wide entry against today's block at shapes both take ----------------------------------------------------------------
@pytest.mark.parametrize("shape,R,tail", wc.SHARED_SHAPES, ids=["x".join(map(str, c[0])) for c in wc.SHARED_SHAPES])
def test_wide_entry_is_as_close_to_float64_as_the_narrow_block(shape, R, tail):
    """es <= max(2 eg, 1e-5 max(1, scale)): the bar of test_streamed_feature_block_equals_the_general_block_to_rounding."""
    w, wide = _block(shape, tail=tail)
    _, narrow = _block(shape, tail=tail, wide=False)
    assert wide.wide and not narrow.wide and not wide.tile_epilogue
    M = 515 if not R else 29 * R
    x = _inputs(shape, M, 3 * shape[0] + shape[2])
    g = np.random.RandomState(R + 5).randn(-(-M // R), shape[1]).astype(np.float32) if R else None
    ref = vc.mlp2_ref(x, w, 0, g, R)
    xd, gd = torch.from_numpy(x).cuda(), None if g is None else torch.from_numpy(g).cuda()
    es = float(np.abs(_run(wide, xd, 0, gd, R, blk=wide) - ref).max())
    eg = float(np.abs(_run(narrow, xd, 0, gd, R, blk=narrow) - ref).max())
    print("%s: wide entry %.3g, narrow block %.3g" % (shape, es, eg))
    assert es <= max(2.0 * eg, 1e-5 * max(1.0, float(np.abs(ref).max()))), (shape, es, eg)


# ---- 4. the float32 form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wc.BLOCK_SHAPES, ids=["x".join(map(str, s)) for s in wc.BLOCK_SHAPES])
def test_float32_form_is_float32_gemm_grade(shape):
    """ebc_mlp2_forward_f32 on a wide handle against float64, no further from it than 3x torch's float32 Linear layers on
    the same batch (or 2e-6): the bar of test_float32_block_is_float32_gemm_grade; the first rows of the batch alone are
    held to the batch's bound; two calls give the same bytes."""
    w, blk = _block(shape)
    M = max(wc.F32_ROW_COUNTS)
    x = _inputs(shape, M, shape[0] * 11 + shape[2])
    xd = torch.from_numpy(x).cuda()
    t = torch.from_numpy
    for relu_out in (0, 1):
        ref = vc.mlp2_ref(x, w, relu_out)
        y32 = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(t(x), t(w["w1"]), t(w["b1"]))), t(w["w2"]), t(w["b2"]))
        y32 = (torch.relu(y32) if relu_out else y32).numpy()
        err_torch = float(np.abs(y32.astype(np.float64) - ref).max())
        for m in wc.F32_ROW_COUNTS:
            got = _run(blk.f32, xd[:m], relu_out, blk=blk)
            err = float(np.abs(got - ref[:m]).max())
            assert err <= max(3.0 * err_torch, 2e-6), (shape, relu_out, m, err, err_torch)
            assert np.array_equal(got.view(np.uint32), _run(blk.f32, xd[:m], relu_out, blk=blk).view(np.uint32)), (shape, m)


@pytest.mark.parametrize("shape,R,B", wc.ATTENTION_CASES, ids=["%s_R%d" % ("x".join(map(str, c[0])), c[1]) for c in wc.ATTENTION_CASES])
def test_float32_form_takes_the_group_term_and_the_tail(shape, R, B):
    w, blk = _block(shape, tail=True)
    rs = np.random.RandomState(shape[1] + R)
    M = B * R
    x = _inputs(shape, M, shape[0] + 17 * R)
    g = rs.randn(B, shape[1]).astype(np.float32)
    ref = vc.mlp2_ref(x, w, 0, g, R)
    t = torch.from_numpy
    h = torch.nn.functional.linear(t(x), t(w["w1"]), t(w["b1"])) + t(g).repeat_interleave(R, 0)
    y = torch.relu(torch.nn.functional.linear(torch.relu(h), t(w["w2"]), t(w["b2"])))
    y32 = (y @ t(w["w3"]) + float(w["b3"][0])).numpy()
    err_torch = float(np.abs(y32.astype(np.float64) - ref).max())
    xd, gd = t(x).cuda(), t(g).cuda()
    for m in (M,) + tuple(c for c in wc.F32_ROW_COUNTS if c < M):
        groups = -(-m // R)
        got = _run(blk.f32, xd[:m], 0, gd[:groups], R, blk=blk)
        err = float(np.abs(got - ref[:m]).max())
        assert err <= max(3.0 * err_torch, 2e-6), (shape, R, m, err, err_torch)
        assert np.array_equal(got.view(np.uint32), _run(blk.f32, xd[:m], 0, gd[:groups], R, blk=blk).view(np.uint32))


# ---- 5. the re-pack -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,tail", wc.REPACK_SHAPES, ids=["x".join(map(str, c[0])) for c in wc.REPACK_SHAPES])
def test_wide_block_repacked_on_the_device_equals_the_host_pack(shape, tail):
    """A wide block created with weights A and updated to B on the device gives the bytes of a wide block created with B,
    in both forms (test_block_repacked_on_the_device_equals_the_host_pack on the wide entry)."""
    wb, b = _block(shape, tail=tail, seed=101)
    _, a = _block(shape, tail=tail, seed=202)
    x = torch.from_numpy(_inputs(shape, 515, 9)).cuda()
    assert not np.array_equal(_run(a, x, 1, blk=a), _run(b, x, 1, blk=b))
    t = lambda k: torch.from_numpy(wb[k]).cuda()  # noqa: E731
    a.update([(t("w1"), t("b1")), (t("w2"), t("b2"))], (t("w3").reshape(1, -1), t("b3")) if tail else None)
    torch.cuda.synchronize()
    for relu in (1, 0):
        for form in ("__call__", "f32"):
            ya, yb = _run(getattr(a, form), x, relu, blk=a), _run(getattr(b, form), x, relu, blk=b)
            assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), (shape, relu, form)
    del _blocks[(shape, tail, True, 202)]  # it no longer holds the weights of its seed


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _create(entry, K0, H, O, flags=0):
    from ebcsim import _capi
    lib = _capi.lib()
    w, _ = vc.make_block(max(K0, 1), max(H, 1), max(O, 1))
    h = C.c_void_p()
    rc = getattr(lib, entry)(0, K0, H, O, w["w1"].ctypes.data, w["b1"].ctypes.data, w["w2"].ctypes.data, w["b2"].ctypes.data, None, None,
                             flags, C.byref(h))
    return rc, h, lib.ebc_last_error()


def test_creation_refusals():
    from ebcsim import _abi, _capi
    for bad in (641, 0):
        for dim in range(3):
            shape = [64, 64, 64]
            shape[dim] = bad
            rc, h, msg = _create("ebc_mlp2_create_wide", *shape)
            assert rc == _abi.ERR_UNSUPPORTED and b"1 .. 640" in msg and not h.value, (shape, rc, msg)
    rc, h, msg = _create("ebc_mlp2_create_wide", 64, 64, 64, flags=_abi.MLP_IN_FRAGMENTS)
    assert rc == _abi.ERR_UNSUPPORTED and b"wide" in msg and b"EBC_MLP_IN_FRAGMENTS" in msg and not h.value, msg
    rc, h, msg = _create("ebc_mlp2_create_ex", 64, 321, 64)  # the narrow entry keeps its limit
    assert rc == _abi.ERR_UNSUPPORTED and not h.value, msg
    rc, h, msg = _create("ebc_mlp2_create_wide", 640, 640, 640)  # the limits themselves are taken
    assert rc == _abi.OK and h.value
    assert _capi.lib().ebc_mlp2_destroy(h) == _abi.OK
    from ebcsim.mlp2 import Mlp2Block
    w, _ = vc.make_block(64, 64, 64)
    t = torch.from_numpy
    with pytest.raises(_capi.EbcError) as err:
        Mlp2Block([(t(w["w1"]), t(w["b1"])), (t(w["w2"]), t(w["b2"]))], 0, in_fragments=True, wide=True)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "wide" in str(err.value)


def test_forward_refusals_write_nothing_and_leave_the_handle_usable():
    """Every argument a wide handle refuses, by name: EBC_ERR_UNSUPPORTED with `wide` in the message, every output
    untouched, and the next good call right; then a stream under capture that would have to allocate the scratch."""
    from ebcsim import _abi, _capi
    from ebcsim.mlp2 import Mlp2Block
    shape = (400, 400, 200)
    w, blk = _block(shape)
    M = 77
    x = _inputs(shape, M, 4)
    xd = torch.from_numpy(x).cuda()
    ref = vc.mlp2_ref(x, w, 0)
    bar = 4e-5 * max(float(np.abs(ref).max()), 1.0)

    def good():
        assert float(np.abs(_run(blk, xd, 0, blk=blk) - ref).max()) <= bar

    good()
    frag = Guarded(((M + 31) // 32, (shape[2] + 31) // 32, 2, 2, 64, 4), torch.int32, tile_rows=1)
    frag_in = Mlp2Block.frag_buffer(M, shape[0], xd.device).zero_()
    weight = torch.ones(M, device=DEV)
    refused = (("frag_in", dict(frag_in=frag_in)), ("frag_out", dict(x=xd, frag_out=frag.t)),
               ("partial", dict(x=xd, want_partial=True, seg_rows=18)), ("seg_rows", dict(x=xd, seg_rows=18)),
               ("row_weight", dict(x=xd, row_weight=weight)), ("EBC_MLP_GENERAL_KERNEL", dict(x=xd, general=True)))
    for word, kw in refused:
        y, part = _y(blk, M), Guarded(((M + 31) // 32, 3, shape[2]), torch.float64, tile_rows=1)
        if kw.get("want_partial"):
            kw = dict(kw, partial_out=part.t)
        with pytest.raises(_capi.EbcError) as err:
            blk.forward_ex(M, False, y_out=y.t, **kw)
        assert err.value.code == _abi.ERR_UNSUPPORTED and "wide" in str(err.value) and word in str(err.value), (word, str(err.value))
        torch.cuda.synchronize()
        for buf in (y, part, frag):
            buf.check(written=False)
        good()
    with pytest.raises(_capi.EbcError) as err:
        blk.reduce(xd, False, 18)
    assert err.value.code == _abi.ERR_UNSUPPORTED and "wide" in str(err.value)
    good()
    # plain rows through ebc_mlp2_forward_ex are ebc_mlp2_forward
    y = _y(blk, M)
    blk.forward_ex(M, False, x=xd, y_out=y.t)
    torch.cuda.synchronize()
    assert np.array_equal(y.check().view(np.uint32), _run(blk, xd, 0, blk=blk).view(np.uint32))

    # a stream the block has not run on: its scratch would have to be allocated inside the capture
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    y, y32 = _y(blk, M), _y(blk, M)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            for entry, buf in ((blk, y), (blk.f32, y32)):
                with pytest.raises(_capi.EbcError) as err:
                    entry(xd, False, out=buf.t)
                assert err.value.code == _abi.ERR_UNSUPPORTED and "wide" in str(err.value) and "capture" in str(err.value)
        finally:
            graph.capture_end()
        side.synchronize()
        y.check(written=False)
        y32.check(written=False)
        blk(xd, False, out=y.t)
        side.synchronize()
    assert float(np.abs(y.check() - ref).max()) <= bar


# ---- 7. whole networks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims,T", wc.NETWORKS, ids=[n[0] for n in wc.NETWORKS])
def test_whole_network_with_wide_blocks_against_float64(name, dims, T):
    """test_whole_network_against_float64's body with wide=True: coarse <= 5e-5, exact <= max(3 e32, 2e-6 max(1, scale));
    one coarse forward moves native_forwards by 1 and folded_forwards by 0, one exact forward native_exact_forwards by 1.
    x2 is all narrow: the counters and the bytes of the network without the keyword."""
    from ebcsim.sarl import SarlValueNet, plan_blocks, plan_facts
    sd = vc.network_state_dict(dims, T, seed=T * 13 + len(name))
    net = SarlValueNet(sd, device=DEV, wide=True)
    cpu64 = SarlValueNet(sd, device="cpu", dtype=torch.float64)
    cpu32 = SarlValueNet(sd, device="cpu")
    narrow_net = SarlValueNet(sd, device=DEV) if name.startswith("x2") else None
    counters = lambda n: (n.native_forwards, n.folded_forwards, n.native_exact_forwards, n.native_exact_mlp1_forwards)  # noqa: E731
    g = torch.Generator().manual_seed(T)
    B = 37
    for R in vc.NETWORK_ROWS:
        rows = torch.randn(B, R, T, generator=g)
        nv = torch.randint(1, R + 1, (B,), generator=g)
        ref = cpu64.forward(rows.double(), nv)
        e32 = float((cpu32.forward(rows, nv).double() - ref).abs().max())
        scale = float(ref.abs().max())
        c0 = counters(net)
        coarse = net.forward(rows.cuda(), nv.cuda())
        c1 = counters(net)
        exact = net.forward(rows.cuda(), nv.cuda(), exact=True)
        c2 = counters(net)
        if narrow_net is None:
            assert tuple(a - b for a, b in zip(c1, c0)) == (1, 0, 0, 0), (name, R, c0, c1)
        else:
            n0 = counters(narrow_net)
            assert torch.equal(coarse, narrow_net.forward(rows.cuda(), nv.cuda())), (name, R)
            assert torch.equal(exact, narrow_net.forward(rows.cuda(), nv.cuda(), exact=True)), (name, R)
            assert tuple(a - b for a, b in zip(counters(narrow_net), n0)) == tuple(a - b for a, b in zip(c2, c0)), (name, R)
        assert tuple(a - b for a, b in zip(c2, c1)) == (0, 0, 1, 0), (name, R, c1, c2)
        ec, ee = float((coarse.double().cpu() - ref).abs().max()), float((exact.double().cpu() - ref).abs().max())
        print("%s R %d: coarse error %.3g, exact error %.3g, float32 CPU %.3g, scale %.3g" % (name, R, ec, ee, e32, scale))
        assert ec <= 5e-5, (name, R, ec)
        assert ee <= max(3.0 * e32, 2e-6 * max(1.0, scale)), (name, R, ee, e32)
    # the blocks are what the plan says, and the facts select_path reads are the plan's
    shapes = wc.stack_shapes(dims, T)
    kinds, gterm = plan_blocks(*shapes, True)
    assert [b.wide for b in net._native] == [k == "wide" for k in kinds] and net._gterm_block.wide == (gterm == "wide")
    assert net._facts == plan_facts((kinds, gterm), shapes[0], shapes[1])
    assert bool(net._native_frag) == ("wide" not in kinds[:3])
    if name.startswith("hidden512"):  # a wide mlp1 beside today's narrow blocks
        assert [b.wide for b in net._native] == [True, False, False, False, False] and not net._gterm_block.wide
        assert all(type(b) is type(net._native[0]) for b in net._native) and net._native[1].tile_epilogue


# ---- 8. decisions ---------------------------------------------------------------------------------------------------------------
DECISION_SEED = 3  # of the x4 network's weights; chosen by the torch path alone (the count of envs left out below)


def test_decisions_with_wide_blocks_are_the_torch_paths():
    """DeviceSarlPolicy on an x4 network with wide=True against the same weights with wide=False (torch's float32 GEMMs): 16
    envs of a device-generated sarl_a5 batch, 81 actions, three consecutive steps.  The action is the same in every env
    whose top two torch values lie further apart than 4x the exact bar of the whole-network test (at most 1 env in 20 may
    be left out on that ground); the values lie within coarse_eps of torch's; the refinement reports no bound violation;
    and, with the bound set to 1e-3 through action_values' own `eps`, it re-evaluates candidates in float32 and still
    reports none."""
    from ebcsim import _abi
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    from test_sarl_train_gpu import _generated_env
    env, space = _generated_env(16)
    sd = vc.network_state_dict(wc.X4, env.T, seed=DECISION_SEED)
    wide, plain = SarlValueNet(sd, device=DEV, wide=True), SarlValueNet(sd, device=DEV)
    cpu64, cpu32 = SarlValueNet(sd, device="cpu", dtype=torch.float64), SarlValueNet(sd, device="cpu")
    pw, pt = DeviceSarlPolicy(wide, space, 0.9), DeviceSarlPolicy(plain, space, 0.9)
    outs = env.alloc_step_outputs(("reward", "done", "info", "dmin"))
    left_out = decisions = 0
    for step in range(3):
        at, vt = pt.decide(env)
        at, vt = at.clone(), vt.clone()
        aw, vw = pw.decide(env)
        torch.cuda.synchronize()
        rows = pw._bufs["rows_rotated"]
        E, A, R, T = rows.shape
        flat = rows.reshape(E * A, R, T).cpu()
        ref = cpu64.forward(flat.double())
        e32 = float((cpu32.forward(flat).double() - ref).abs().max())
        bar = max(3.0 * e32, 2e-6 * max(1.0, float(ref.abs().max())))
        top = torch.topk(vt, 2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 4.0 * bar
        left_out += int((~clear).sum())
        decisions += E
        assert torch.equal(aw[clear], at[clear]), (step, int((aw != at).any(1).sum()))
        worst = float((vw - vt).abs().max())
        print("step %d: %d of %d envs clear, values within %.3g of torch's, coarse_eps %.3g" % (step, int(clear.sum()), E, worst, wide.coarse_eps))
        assert worst <= wide.coarse_eps, (step, worst, wide.coarse_eps)
        env.step_device(outs, robot_action=at.contiguous(), human_policy=_abi.HUMAN_CACHED)
    assert 20 * left_out <= decisions, (left_out, decisions)
    assert plain.native_forwards == 0 and wide.native_forwards > 0 and wide.native_exact_forwards > 0
    st = wide.refine_stats
    assert st["decisions"] == decisions and st["bound_violations"] == 0 and st["fallbacks"] == 0, st
    # a wider bound: many candidates per env go through the float32 form of the wide blocks
    rows, reward = pw._bufs["rows_rotated"], pw._bufs["reward"]
    values = wide.action_values(rows, reward, 0.9, eps=1e-3)
    torch.cuda.synchronize()
    st = wide.refine_stats
    assert st["candidates"] > 0 and st["bound_violations"] == 0 and st["fallbacks"] == 0, st
    assert bool(torch.isfinite(values).all())
    env.close()


# ---- 9. the schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_decide", [True, False])
def test_training_schedule_decides_with_wide_blocks(tmp_path, wide_decide):
    """run_sarl_training(_ex) on 64 envs with the x3 network (grad_form="auto": the layer form): 4 imitation steps, 1 epoch, 2
    RL rounds.  With wide_decide the rollouts' network ran on its blocks and was refreshed from the trainer; without it
    the same call leaves native_forwards at 0 (torch)."""
    from sarl_grad_cases import module
    from ebcsim.sarl_train import SarlFormTrainer, run_sarl_training, run_sarl_training_ex
    from test_sarl_train_gpu import _generated_env
    env, space = _generated_env(64)
    net = ([env.T, 400, 300, 300, 100, 300, 300, 1, 400, 300, 300, 1], 6, True)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(21)
        tr = SarlFormTrainer(module(net), device=DEV, optimizer="sgd", lr=0.01, grad_form="auto")
    assert tr.net.form == "layers"
    kw = {"wide_decide": True} if wide_decide else {}
    hist = (run_sarl_training_ex if wide_decide else run_sarl_training)(env, tr, space, 0.9, il_steps=4, il_epochs=1, train_iterations=2, steps_per_iteration=30, train_batches=2,
                             batch_size=16, capacity=4096, epsilon_start=0.5, epsilon_end=0.5, target_update_interval=1,
                             generator=torch.Generator(device=DEV).manual_seed(5), output_dir=str(tmp_path), **kw)
    env.close()
    assert len(hist["rl_loss"]) == 2 and np.isfinite(hist["mean_reward"]).all()
    assert hist["memory"] > 0 and np.isfinite(hist["rl_loss"][-1]), hist  # some episode ended within the 60 decisions
    assert all(bool(torch.isfinite(v).all()) for v in tr.state_dict().values())
    if wide_decide:
        assert hist["native_refreshes"] > 0 and hist["native_forwards"] > 0, hist
    else:
        assert hist["native_forwards"] == 0, hist
