"""The two-layer value-network blocks at every compiled tile shape (csrc/ebc_value_net.h, csrc/ebc_vn_stream.h) against
float64 evaluations of the same rows: the case tables and references of tests/value_net_cases.py, run on the device.
tests/test_value_net_shapes_cpu.py asserts that the tables reach what they claim.  Bars are those of
tests/test_value_net.py; every buffer a kernel writes is a guarded one (tests/helpers.py: Guarded), poisoned where the
call must write all of it; what a form refuses is named in the table and must leave its outputs untouched."""
import numpy as np
import pytest
import torch

import value_net_cases as vc
from helpers import Guarded
from test_value_net import _frag, _part, _y

pytestmark = pytest.mark.gpu
LATTICE = [(TI, TO) for TI in range(1, 8) for TO in range(1, 8)]


def _lib():
    from ebcsim import _capi
    return _capi.lib()


def _native(w, in_fragments=False):
    from ebcsim.sarl import _NativeMlp2
    t = torch.from_numpy
    fin = (t(w["w3"])[None, :], t(w["b3"])) if "w3" in w else None
    return _NativeMlp2([(t(w["w1"]), t(w["b1"])), (t(w["w2"]), t(w["b2"]))], 0, final=fin, in_fragments=in_fragments)


def _assert_rows(got, ref, what):
    """Split-bf16 rows against float64: three bf16 products per float32 product, 4e-5 of the scale."""
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= 4e-5 * max(scale, 1.0), (what, err, scale)


def _frag_rows(frag_i32, M, width):
    """A hand-off tensor (host int32) read back as rows: hi + lo of every element."""
    f = torch.from_numpy(np.ascontiguousarray(frag_i32)).view(torch.bfloat16).float()  # [tile][column tile][k-step][hi, lo][lane][8]
    return vc.frag_unpack((f[:, :, :, 0] + f[:, :, :, 1]).numpy(), M, width)


class _PairSums(object):
    """The buffers of one epilogue call on M rows in groups of R: the rows' weights (ebc_pair_mask of ragged counts, or
    none), the partial sums — as many tiles as WHOLE groups span, so that ebc_pair_combine may read a last group that M
    cuts short: the tiles past M hold zeros, the kernel owes the others — and the combined sums."""

    def __init__(self, rs, M, R, O, ragged, refused):
        self.M, self.R, self.B, self.O = M, R, -(-M // R), O
        self.tiles = (M + 31) // 32
        self.nv = rs.randint(1, R + 1, size=self.B).astype(np.int64) if ragged else None
        self.nvd = None if self.nv is None else torch.from_numpy(self.nv).cuda()
        self.mask = None
        if ragged:
            self.mask = Guarded((self.B * R,), torch.float32)
            from ebcsim import _capi
            _capi.check(_lib().ebc_pair_mask(None, self.nvd.data_ptr(), self.B, R, self.mask.t.data_ptr()))
        self.part = _part(self.B * R, O)
        if not refused:
            self.part.t[self.tiles:] = 0
        self.weight = None if self.mask is None else self.mask.t

    def combined(self, mean):
        """ebc_pair_combine of the partial sums (checked) -> [B][O] on the host."""
        from ebcsim import _capi
        out = Guarded((self.B, self.O), torch.float32)
        nvp = None if self.nvd is None else self.nvd.data_ptr()
        _capi.check(_lib().ebc_pair_combine(None, self.part.t.data_ptr(), nvp, self.B, self.R, self.O, int(mean), out.t.data_ptr()))
        torch.cuda.synchronize()
        self.part.check()
        if self.mask is not None:
            self.mask.check()
        return out.check()

    def assert_sums(self, got, rows, weight=None, mean=True, what=None):
        """Pair sums against the float64 sums of the rows themselves, to float32 rounding."""
        rows = np.asarray(rows, np.float64)
        want = vc.pair_sums_ref(rows, self.R, self.M, self.nv, weight, mean)
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6 * float(np.abs(rows).max()), err_msg=str(what))

    def untouched(self):
        torch.cuda.synchronize()
        self.part.check(written=False)


# ---- part 1: the general block over its lattice ------------------------------------------------------------------------
def _rows_case(c):
    from ebcsim import _capi
    L = _lib()
    tail, group, reduce = "tail" in c["form"], "group" in c["form"], "reduce" in c["form"]
    K0, H, O = c["K0"], c["H"], c["O"]
    w, rs = vc.make_block(K0, H, O, tail)
    blk = _native(w)
    x = (rs.randn(max(c["Ms"]), K0) * 2).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    Rg = c["group_rows"] if group else 0
    rb = rs.randn(-(-max(c["Ms"]) // Rg), H).astype(np.float32) if group else None
    for M in c["Ms"]:
        what = (c["form"], K0, H, O, M)
        rbm = None if rb is None else rb[:-(-M // Rg)]
        plain = _y(blk, M)
        blk(xd[:M], c["relu"], row_bias=None if rbm is None else torch.from_numpy(rbm).cuda(), group_rows=Rg, out=plain.t)
        torch.cuda.synchronize()
        rows = plain.check()
        _assert_rows(rows, vc.mlp2_ref(x[:M], w, c["relu"], rbm, Rg), what)
        if not reduce:
            continue
        store = "reduce_y" in c["form"]
        ps = _PairSums(rs, M, c["seg_rows"], O, c["ragged"], c["refused"])
        yg = Guarded((M, O), torch.float32)
        rc = L.ebc_mlp2_forward_reduce(blk._h, None, xd.data_ptr(), M, c["relu"], None, 0, yg.t.data_ptr() if store else None,
                                       c["seg_rows"], None if ps.weight is None else ps.weight.data_ptr(), ps.part.t.data_ptr())
        if c["refused"]:
            assert rc == -2 and c["refused"] in L.ebc_last_error().decode(), (what, rc, L.ebc_last_error())
            ps.untouched()
            yg.check(written=False)
            continue
        _capi.check(rc)
        got = ps.combined(mean=True)
        if store:
            np.testing.assert_array_equal(yg.check(), rows, err_msg=str(what))  # the same kernel, the same bits
        else:
            yg.check(written=False)
        ps.assert_sums(got, rows, what=what)


@pytest.mark.parametrize("TI,TO", LATTICE)
def test_general_block_row_forms(TI, TO):
    """Every input width at the edges of tile TI and of its k-steps, with 32 TO, 32 (TO - 1) + 4 and an odd number of
    outputs: the plain store with and without ReLU, the per-group term, the one-output tail, both together, and the
    row-group sums with and without the rows — at one row, both sides of a tile, exactly one workgroup, and two
    workgroups and a row."""
    for c in vc.block_cases(TI, TO):
        if c["kind"] == "rows":
            _rows_case(c)


def _chain_case(c):
    from ebcsim import _capi
    K0, H, O, R = c["K0"], c["H"], c["O"], c["seg_rows"]
    w, rs = vc.make_block(K0, H, O)
    src = _native(w)
    d = c["consumer"]
    wc, _ = vc.make_block(d["K0"], d["H"], d["O"], "tail" in d["form"])
    con = _native(wc, in_fragments=True)
    x = (rs.randn(max(c["Ms"]), K0) * 2).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    for M in c["Ms"]:
        what = ("chain", K0, H, O, M)
        plain = _y(src, M)
        src(xd[:M], True, out=plain.t)
        torch.cuda.synchronize()
        rows = plain.check()
        _assert_rows(rows, vc.mlp2_ref(x[:M], w, 1), what)
        # the `mlp1` form: rows in; fragments and masked pair sums out; the rows themselves never written
        ps = _PairSums(rs, M, R, O, True, c["refused"])
        frag = _frag(M, O)

        def produce():
            src.forward_ex(M, True, x=xd[:M], want_y=False, seg_rows=R, row_weight=ps.weight, want_partial=True, frag_out=frag.t,
                           general=True, partial_out=ps.part.t[:ps.tiles])
        if c["refused"]:
            with pytest.raises(_capi.EbcError, match=c["refused"]):
                produce()
            ps.untouched()
            frag.check(written=False)
            handed = vc.frag_pack(rows)  # the consumers' input all the same: the rows split on the host
        else:
            produce()
            ps.assert_sums(ps.combined(mean=True), rows, what=what)
            handed = torch.from_numpy(frag.check().copy())
            d_rows = float(np.abs(_frag_rows(handed.numpy(), M, O) - rows).max())
            assert d_rows <= 2e-5 * max(1.0, float(np.abs(rows).max())), (what, d_rows)
        # the consumers, the general kernel: what they multiply is hi + lo of the tensor they were handed
        xin = _frag_rows(handed.numpy(), M, O)
        hd = (frag.t if not c["refused"] else handed.cuda())
        whatc = ("consumer", d["form"], d["K0"], d["H"], d["O"], M)
        if d["form"] == "group+tail":
            Rg = d["group_rows"]
            rb = rs.randn(-(-M // Rg), d["H"]).astype(np.float32)
            ya = _y(con, M)
            con.forward_ex(M, False, frag_in=hd, row_bias=torch.from_numpy(rb).cuda(), group_rows=Rg, general=True, y_out=ya.t)
            torch.cuda.synchronize()
            _assert_rows(ya.check(), vc.mlp2_ref(xin, wc, 0, rb, Rg), whatc)
            continue
        wt = rs.rand(-(-M // R) * R).astype(np.float32)
        wd = torch.from_numpy(wt).cuda()
        pc = _PairSums(rs, M, R, d["O"], False, d["refused"])

        def consume(want_y, y_out=None):
            con.forward_ex(M, False, frag_in=hd, want_y=want_y, seg_rows=R, row_weight=wd, want_partial=True, general=True,
                           y_out=y_out, partial_out=pc.part.t[:pc.tiles])
        if d["refused"]:
            with pytest.raises(_capi.EbcError, match=d["refused"]):
                consume(False)
            pc.untouched()
            continue
        yc = _y(con, M)
        consume(True, yc.t)  # with the rows: they are what the sums are held to
        crows = yc.check()
        _assert_rows(crows, vc.mlp2_ref(xin, wc, 0), whatc)
        first = pc.combined(mean=False)
        pc.assert_sums(first, crows, weight=wt, mean=False, what=whatc)
        pc.part.t[:pc.tiles].view(torch.uint8).fill_(Guarded.POISON)
        consume(False)      # `mlp2` as SarlValueNet calls it: the weighted sums alone
        np.testing.assert_array_equal(pc.combined(mean=False), first, err_msg=str(whatc))


@pytest.mark.parametrize("TI,TO", LATTICE)
def test_general_block_handoff_chain(TI, TO):
    """The block as SarlValueNet's `mlp1` (rows in; fragments and masked pair sums out) at an input width on either side of
    tile TI's k-step boundary, and the consumers of its fragments — the transposed pair (TO, TI) as the attention stack
    (group term, one-output tail) and as `mlp2` (weighted pair sums, no rows) — on the general kernel."""
    for c in vc.block_cases(TI, TO):
        if c["kind"] == "chain":
            _chain_case(c)


# ---- part 2: the float32 forms ---------------------------------------------------------------------------------------------
def _f32_case(c, tails):
    K0, H, O, M, Rg = c["K0"], c["H"], c["O"], c["M"], c["group_rows"]
    w, _ = vc.make_block(K0, H, O, c["tail"])
    blk = _native(w)
    g = torch.Generator().manual_seed(K0 * 7 + O)
    x = torch.randn(M, K0, generator=g)
    rb = torch.randn(-(-M // Rg), H, generator=g) if Rg else None
    t = {k: torch.from_numpy(v) for k, v in w.items()}

    def ref(dt):
        h = torch.nn.functional.linear(x.to(dt), t["w1"].to(dt), t["b1"].to(dt))
        if rb is not None:
            h = h + rb.to(dt).repeat_interleave(Rg, 0)[:M]
        y = torch.nn.functional.linear(torch.relu(h), t["w2"].to(dt), t["b2"].to(dt))
        if c["tail"]:
            return torch.nn.functional.linear(torch.relu(y), t["w3"].to(dt)[None, :], t["b3"].to(dt)).squeeze(1)
        return torch.relu(y) if c["relu"] else y
    exact = ref(torch.float64)
    err_torch = float((ref(torch.float32).double() - exact).abs().max())
    xd = x.cuda()
    for m in (M,) + tuple(tails):
        yg = _y(blk, m)
        blk.f32(xd[:m], c["relu"], row_bias=None if rb is None else rb[:-(-m // Rg)].cuda(), group_rows=Rg, out=yg.t)
        torch.cuda.synchronize()
        err = float((torch.from_numpy(yg.check()).double() - exact[:m]).abs().max())
        print("f32 %s K0 %d H %d O %d rows %d: error %.3g, torch float32 %.3g" % (c["form"], K0, H, O, m, err, err_torch))
        assert err <= max(3.0 * err_torch, 2e-6), (c, m, err, err_torch)


@pytest.mark.parametrize("c", vc.F32_FEW, ids=lambda c: "K%d-H%d-O%d" % (c["K0"], c["H"], c["O"]))
def test_float32_tile_form_over_the_widths(c):
    """ebc_mlp2_forward_f32 on few rows (a workgroup per tile) at every input-width edge of 1, 3 and 7 tiles."""
    _f32_case(c, vc.F32_FEW_TAILS)


@pytest.mark.parametrize("c", vc.F32_MANY, ids=lambda c: "T2_%d-K%d-H%d-O%d" % (c["T2"], c["K0"], c["H"], c["O"]))
def test_float32_row_form_at_every_output_tile_count(c):
    """mlp2_f32_kernel<T2> for T2 = 1 .. 7, reached with one row more than the tile form takes."""
    _f32_case(c, ())


# ---- part 3: the streamed kernels off their one tested width -----------------------------------------------------------------
def _first_block(K0, H, O, B, general_pair):
    """`mlp1` as SarlValueNet calls it on B ragged pairs of 18 rows, default selector and EBC_MLP_GENERAL_KERNEL ->
    {general: (pair sums, hi + lo of the fragments)}, the float64 pair sums, the largest |row| value."""
    from ebcsim.sarl import SarlValueNet
    R, M = 18, B * 18
    w, rs = vc.make_block(K0, H, O)
    blk = _native(w)
    x = (rs.randn(M, K0) * 2).astype(np.float32)
    nv = rs.randint(12, R + 1, size=B)
    mask = (np.arange(R)[None, :] < nv[:, None]).astype(np.float32).reshape(M)
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    out, guards = {}, []
    for general in general_pair:
        frag, part, comb = _frag(M, O), _part(M, O), Guarded((B, O), torch.float32)
        blk.forward_ex(M, True, x=xd, want_y=False, seg_rows=R, row_weight=md, want_partial=True, frag_out=frag.t, general=general,
                       partial_out=part.t)
        SarlValueNet._pair_combine(part.t, None, B, R, False, out=comb.t)
        guards.append((frag, part, comb))
    torch.cuda.synchronize()
    for general, (frag, part, comb) in zip(general_pair, guards):
        part.check()
        out[general] = (comb.check(), _frag_rows(frag.check(), M, O))
    rows = vc.mlp2_ref(x, w, 1)
    return out, (rows * mask[:, None]).reshape(B, R, O).sum(1), float(np.abs(rows).max())


@pytest.mark.parametrize("K0", (17, 20, 29, 31, 32))
def test_streamed_first_block_off_its_width(K0):
    """The streamed `mlp1` at the OM-SARL widths and on both sides of KH (hidden width 32 * 10 - 16) against the general
    block (another order of the hidden sums) and float64, at the bars of
    test_streamed_first_block_equals_the_general_block_to_rounding: three workgroups the last of which is part-filled,
    and one pair."""
    for (k, H, O) in vc.STREAM_FIRST:
        if k != K0:
            continue
        for B in (29, 1):
            out, ref, _ = _first_block(K0, H, O, B, (False, True))
            es, eg = float(np.abs(out[False][0] - ref).max()), float(np.abs(out[True][0] - ref).max())
            assert es <= max(2.0 * eg, 1e-5 * max(1.0, float(np.abs(ref).max()))), (K0, H, O, B, es, eg)
            d = float(np.abs(out[False][1] - out[True][1]).max())
            assert d <= 2e-5 * max(1.0, float(np.abs(out[True][1]).max())), (K0, H, O, B, d)
            assert float(np.abs(out[False][1]).max()) > 0


@pytest.mark.parametrize("K0,H,O", vc.STREAM_FIRST_GENERAL)
def test_first_block_of_half_a_tile_takes_the_general_kernel(K0, H, O):
    """K0 <= 16 is not the streamed kernel's: the default selector and EBC_MLP_GENERAL_KERNEL run the same kernel, so the
    pair sums and the fragments are the same bits."""
    for B in (29, 1):
        out, ref, scale = _first_block(K0, H, O, B, (False, True))
        np.testing.assert_array_equal(out[False][0], out[True][0])
        np.testing.assert_array_equal(out[False][1], out[True][1])
        # a pair's sum of up to 18 rows, each within the split-bf16 bar of its float64 value
        assert float(np.abs(out[True][0] - ref).max()) <= 18 * 4e-5 * max(1.0, scale)


def _handed_rows(rs, M, K0):
    """Non-negative rows like h1 and their hand-off tensor, split on the host (an odd width has no producer: frag_out
    wants a multiple of 4) -> (device tensor, hi + lo of it as rows)."""
    handed = vc.frag_pack(np.abs(rs.randn(M, K0)).astype(np.float32))
    return handed.cuda(), _frag_rows(handed.numpy(), M, K0)


@pytest.mark.parametrize("K0,H,O", vc.STREAM_ATTENTION)
def test_streamed_attention_block_at_the_kstep_boundary(K0, H, O):
    """The attention block with K0 and H on both sides of 32 * 7 - 16 (KIN / KH): bit-equal to the general block, and
    both within the split-bf16 bar of float64.  (H = 209: the group terms cannot be parked, the selector itself takes the
    general kernel.)"""
    w, rs = vc.make_block(K0, H, O, tail=True)
    blk = _native(w, in_fragments=True)
    for M in (18 * 57 + 5, 31, 32 * 8 * 3 + 1, 18):
        hd, xin = _handed_rows(rs, M, K0)
        rb = rs.randn(-(-M // 18), H).astype(np.float32)
        rbd = torch.from_numpy(rb).cuda()
        ya, yb = _y(blk, M), _y(blk, M)
        blk.forward_ex(M, False, frag_in=hd, row_bias=rbd, group_rows=18, y_out=ya.t)
        blk.forward_ex(M, False, frag_in=hd, row_bias=rbd, group_rows=18, general=True, y_out=yb.t)
        torch.cuda.synchronize()
        a, b = ya.check(), yb.check()
        np.testing.assert_array_equal(a, b, err_msg=str((K0, H, O, M)))
        _assert_rows(b, vc.mlp2_ref(xin, w, 0, rb, 18), ("attention", K0, H, O, M))


@pytest.mark.parametrize("K0,H,O", vc.STREAM_FEATURE)
def test_streamed_feature_block_at_the_kstep_boundary(K0, H, O):
    """`mlp2` streamed with K0 and H on both sides of 32 * 7 - 16 against the general block and float64, at the bar of
    test_streamed_feature_block_equals_the_general_block_to_rounding."""
    from ebcsim.sarl import SarlValueNet
    R = 18
    w, rs = vc.make_block(K0, H, O)
    blk = _native(w, in_fragments=True)
    for B in (57, 1):
        M = B * R
        hd, xin = _handed_rows(rs, M, K0)
        wt = rs.rand(M).astype(np.float32)
        wd = torch.from_numpy(wt).cuda()
        out = {}
        for general in (False, True):
            part, comb = _part(M, O), Guarded((B, O), torch.float32)
            blk.forward_ex(M, False, frag_in=hd, want_y=False, seg_rows=R, row_weight=wd, want_partial=True, general=general,
                           partial_out=part.t)
            SarlValueNet._pair_combine(part.t, None, B, R, False, out=comb.t)
            torch.cuda.synchronize()
            part.check()
            out[general] = comb.check()
        ref = (vc.mlp2_ref(xin, w, 0) * wt.astype(np.float64)[:, None]).reshape(B, R, O).sum(1)
        es, eg = float(np.abs(out[False] - ref).max()), float(np.abs(out[True] - ref).max())
        assert es <= max(2.0 * eg, 1e-5 * max(1.0, float(np.abs(ref).max()))), (K0, H, O, B, es, eg)


# ---- part 4: whole networks of other shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims,T,native,native_exact", vc.NETWORKS, ids=[n[0] for n in vc.NETWORKS])
def test_whole_network_against_float64(name, dims, T, native, native_exact):
    """SarlValueNet.forward on the device against the same class on the CPU in float64 (test_sarl_values_cpu pins that
    path to the reference's recorded values): random weights, ragged pairs, pair sizes on both sides of the folded
    path's 16 .. 32.  Coarse values within DESIGN section 4's 5e-5; exact=True values as good as a float32 CPU run; the
    counters say which path ran — a network the blocks do not take falls back and says so."""
    from ebcsim.sarl import SarlValueNet
    sd = vc.network_state_dict(dims, T, seed=T * 13 + len(name))
    net = SarlValueNet(sd, device="cuda:0")
    cpu64 = SarlValueNet(sd, device="cpu", dtype=torch.float64)
    cpu32 = SarlValueNet(sd, device="cpu")
    g = torch.Generator().manual_seed(T)
    B = 37
    for R in vc.NETWORK_ROWS:
        rows = torch.randn(B, R, T, generator=g)
        nv = torch.randint(1, R + 1, (B,), generator=g)
        ref = cpu64.forward(rows.double(), nv)
        e32 = float((cpu32.forward(rows, nv).double() - ref).abs().max())
        scale = float(ref.abs().max())
        before = (getattr(net, "native_forwards", 0), getattr(net, "native_exact_forwards", 0))
        coarse = net.forward(rows.cuda(), nv.cuda()).double().cpu()
        mid = (getattr(net, "native_forwards", 0), getattr(net, "native_exact_forwards", 0))
        exact = net.forward(rows.cuda(), nv.cuda(), exact=True).double().cpu()
        after = (getattr(net, "native_forwards", 0), getattr(net, "native_exact_forwards", 0))
        assert (mid[0] - before[0], mid[1] - before[1]) == (native, 0), (name, R, before, mid)
        assert (after[0] - mid[0], after[1] - mid[1]) == (0, native_exact), (name, R, mid, after)
        ec, ee = float((coarse - ref).abs().max()), float((exact - ref).abs().max())
        print("%s R %d: coarse error %.3g, exact error %.3g, float32 CPU %.3g, scale %.3g" % (name, R, ec, ee, e32, scale))
        assert ec <= 5e-5, (name, R, ec)
        assert ee <= max(3.0 * e32, 2e-6 * max(1.0, scale)), (name, R, ee, e32)


# what each path of ebcsim.sarl.select_path adds to (native_forwards, folded_forwards, native_exact_forwards,
# native_exact_mlp1_forwards)
PATH_COUNTERS = {"folded_frag": (1, 1, 0, 0), "folded_rows": (1, 1, 0, 0), "blocks": (1, 0, 0, 0),
                 "exact_native": (0, 0, 1, 0), "exact_mlp1": (0, 0, 0, 1), "torch": (0, 0, 0, 0)}


@pytest.mark.parametrize("which", ("golden", "small_T13"))
def test_the_counters_follow_the_selector(which):
    """One forward moves exactly the counters of the path the selector names, by 1: the shipped weights (folded between
    16 and 32 rows, the library's float32 form when exact) and the network whose blocks have no tile epilogue."""
    import os
    from ebcsim.sarl import SarlValueNet
    from helpers import GOLDEN
    if which == "golden":
        net = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device="cuda:0")
    else:
        name, dims, T, _, _ = next(n for n in vc.NETWORKS if n[0] == which)
        net = SarlValueNet(vc.network_state_dict(dims, T, seed=T * 13 + len(name)), device="cuda:0")
    g = torch.Generator().manual_seed(5)
    B, T = 5, net.input_dim
    counters = lambda: (net.native_forwards, net.folded_forwards, net.native_exact_forwards, net.native_exact_mlp1_forwards)  # noqa: E731
    seen = set()
    for R in vc.NETWORK_ROWS:
        rows = torch.randn(B, R, T, generator=g).cuda()
        nv = torch.randint(1, R + 1, (B,), generator=g).cuda()
        for exact in (False, True):
            with torch.no_grad():
                path = net.path_for(rows, exact=exact)
            before = counters()
            out = net.forward(rows, nv, exact=exact)
            moved = tuple(a - b for a, b in zip(counters(), before))
            assert moved == PATH_COUNTERS[path], (which, R, exact, path, moved)
            assert tuple(out.shape) == (B,) and bool(torch.isfinite(out).all())
            seen.add(path)
    assert seen == ({"folded_frag", "blocks", "exact_native"} if which == "golden" else {"blocks", "exact_native"}), seen
