"""What the case tables of tests/value_net_cases.py reach: a property of the TABLES, asserted without a GPU.  The
selector of the two-layer blocks (mlp2_dispatch -> launch_mlp2 -> launch_mlp2_to -> launch_mlp2_kernel in
csrc/ebcsim_value_net.hip, the layout of mlp2_split_wg_kernel in csrc/ebc_vn_layout.h, vn_stream_launch in
csrc/ebcsim_vn_stream.hip) is restated in value_net_cases.py in a few lines; here that restatement is held to a reading
of the arithmetic in closed form, to the layout header's own answers (tests/native/vn_layout_host.cc) and to the
constants in the sources, and the tables to the instantiations, layouts,
input paths and selector branches they are there for.  The conditions are requirements on the tables: when one is
missed, change the table, not the condition.

The counts go to profiles/value_net_shape_coverage.txt."""
import os
import subprocess
from collections import Counter

import numpy as np
import torch

import value_net_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "value_net_shape_coverage.txt")
CSRC = os.path.join(ROOT, "eb-cadrl_amd", "csrc")
LATTICE = [(TI, TO) for TI in range(1, 8) for TO in range(1, 8)]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _layout_program(tmp_path):
    """tests/native/vn_layout_host.cc — csrc/ebc_vn_layout.h as the kernel and the launcher compile it — built with g++ as
    a program of its own under -fsanitize=address,undefined (a finding ends it with a non-zero status); its lines."""
    exe = str(tmp_path / "vn_layout_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "vn_layout_host.cc"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    return r.stdout.splitlines()


def test_the_restated_constants_are_the_sources(tmp_path):
    """The layout of the general block — class, waves, input path, tile epilogue — against what csrc/ebc_vn_layout.h itself
    answers over the whole lattice (every K0 of the input tile; O = 32 TO, 32 (TO - 1) + 4 and 32 TO - 3); the other
    constants against the lines of the sources that hold them."""
    vn, host, stream = _src("ebc_value_net.h"), _src("ebcsim_value_net.hip"), _src("ebcsim_vn_stream.hip")
    lines = _layout_program(tmp_path)
    assert lines[-1] == "EBC_VN_XROW %d EBC_VN_GROUPS %d EBC_VN_GROUP_PITCH %d" % (vc.XROW, vc.VN_GROUPS, vc.VN_GROUP_PITCH)
    assert len(lines) == len(LATTICE) + 1
    for (TI, TO), line in zip(LATTICE, lines):
        ti, to, cls, nw, weights, xcap, region, lds_plain, lds_group, rows, epi = line.split()
        assert (int(ti), int(to)) == (TI, TO) and (cls, int(nw)) == vc.layout(TI, TO), line
        k0s = range(32 * (TI - 1) + 1, 32 * TI + 1)
        assert rows == "rows=" + "".join("1" if vc.input_path(TI, TO, K0) == "lds" else "0" for K0 in k0s), line
        assert epi == "epilogue=" + "".join(str(int(vc.tile_epilogue(TI, TO, O))) for O in (32 * TO, 32 * (TO - 1) + 4, 32 * TO - 3)), line
        # the region the parked tiles take is the weight region; the launch's LDS: + the biases of 7 hidden tiles, + NW waves' group terms
        assert int(region) == int(weights) == ((2 * TI + TO) * 4096 if cls == "lean" else (TI + TO) * 8192), line
        assert int(xcap) == (TI * 4096 if cls == "lean" else (TI + TO) * 4096), line
        assert int(lds_plain) == int(weights) + 7 * 32 * 4 and int(lds_group) == int(lds_plain) + int(nw) * vc.VN_GROUPS * vc.VN_GROUP_PITCH, line
    assert "Hp * 4 + 16 <= EBC_VN_GROUP_PITCH" in vn
    assert "(ex.H & 3) == 0 && ex.group_rows > 0 && (31 / ex.group_rows + 2) <= EBC_VN_GROUPS" in vn
    assert "#define EBC_F32_TILE_ROWS (1 << 16)" in vn and vc.F32_TILE_ROWS == 1 << 16
    assert "K0 > %d || O > %d || H > %d" % (vc.MAX_IN, vc.MAX_OUT, vc.MAX_HIDDEN) in host
    assert "if constexpr (TI == 7) {\n    if (m->K0 <= 32 * TI - 16)" in host
    assert "L1.in_tiles == 1 && K0 > 16 && L1.out_tiles == 10 && L2.out_tiles == 7" in stream
    assert "kin = K0 <= 32 * 7 - 16, kh = H <= 32 * 7 - 16" in stream and "if (H <= 32 * 10 - 16)" in stream


def test_the_selector_in_closed_form():
    """The lean layout iff TI + TO >= 10 and 2 TI + TO <= 19; eight waves only for (7, 6) and (7, 7); rows parked in LDS
    iff TI >= 2, K0 a multiple of 4, and TI + TO >= 5 in the full layout / TI >= 5 in the lean one (8 waves: always); the
    tile epilogue everywhere but at 1 + 1 tiles."""
    for TI, TO in LATTICE:
        cls, NW = vc.layout(TI, TO)
        assert (cls == "lean") == (TI + TO >= 10 and 2 * TI + TO <= 19), (TI, TO)
        assert (NW == 8) == ((TI, TO) in ((7, 6), (7, 7))) and (cls == "full8") == (NW == 8), (TI, TO)
        room = {"full": TI + TO >= 5, "lean": TI >= 5, "full8": True}[cls]
        for K0 in range(32 * (TI - 1) + 1, 32 * TI + 1):
            assert (vc.input_path(TI, TO, K0) == "lds") == (TI >= 2 and K0 % 4 == 0 and room), (TI, TO, K0)
            assert vc.kin(TI, K0) == int(TI == 7 and K0 <= 208)
        assert vc.tile_epilogue(TI, TO, 32 * TO) == (TI + TO >= 3) and not vc.tile_epilogue(TI, TO, 32 * TO - 3)


def _all():
    return {p: vc.block_cases(*p) for p in LATTICE}


def test_part_1_hits_every_instantiation():
    inst = [i for p in LATTICE for i in vc.instantiations(*p)]
    hit = {(TI, TO, G) for TI, TO, NW, G, cls, kin, path in inst}
    assert hit == {(TI, TO, G) for TI, TO in LATTICE for G in (False, True)}
    assert {cls for _, _, _, _, cls, _, _ in inst} == {"full", "lean", "full8"}
    for TI, TO, NW, G, cls, kin, path in inst:
        assert (cls, NW) == vc.layout(TI, TO)
    for TO in range(1, 8):  # both sides of the KIN boundary, with and without the group term, rows and fragments
        for G in (False, True):
            assert {kin for TI, to, NW, g, cls, kin, path in inst if (TI, to, g) == (7, TO, G)} == {0, 1}, (TO, G)
        assert {kin for TI, to, NW, g, cls, kin, path in inst if (TI, to, path) == (7, TO, "frag")} == {0, 1}, TO
    # every input path wherever the kernel has it: per pair, so per layout class too
    for TI, TO in LATTICE:
        has = {"lane", "frag"} | ({"lds"} if vc.input_path(TI, TO, 32 * TI) == "lds" else set())
        assert {path for ti, to, NW, G, cls, kin, path in inst if (ti, to) == (TI, TO)} == has, (TI, TO)
    for cls in ("full", "lean", "full8"):
        for path in ("lane", "lds", "frag"):
            assert any(i[4] == cls and i[6] == path for i in inst), (cls, path)
            assert any(i[4] == cls and i[6] == path and i[3] for i in inst), (cls, path, "with the group term")


def test_part_1_holds_the_edges_it_names():
    cases = _all()
    hidden_by_form, forms_by_ti, gpaths, segs = Counter(), Counter(), Counter(), Counter()
    for (TI, TO), cs in cases.items():
        NW = vc.layout(TI, TO)[1]
        rows = [c for c in cs if c["kind"] == "rows" and c["refused"] != vc.NEEDS_O4]
        assert sorted({c["K0"] for c in rows if c["O"] % 4 == 0}) == vc.k0_edges(TI), (TI, TO)
        assert {c["K0"] % 4 == 0 for c in rows} == {True, False}
        if TI == 7:
            assert {208, 209} <= {c["K0"] for c in rows}
        assert {32 * TO, 32 * (TO - 1) + 4, 32 * TO - 3} == {c["O"] for c in rows}
        for c in rows:
            assert c["O"] % 4 == 0 or c["form"] in ("plain0", "plain1")  # an odd O: the plain store only
        assert {c["form"] for c in rows} == set(vc.FORMS) | {"plain%d" % ((TI + TO) % 2)}
        for c in cs:
            assert set(vc.row_counts(NW)) <= set(c["Ms"]) or c["refused"] == vc.NEEDS_O4
            if c["kind"] == "chain":
                assert set(vc.row_counts(vc.layout(TO, TI)[1])) <= set(c["Ms"])
                assert c["K0"] % 4 in (0, 1) and c["O"] == c["consumer"]["K0"] and c["O"] % 4 == 0
                assert vc.tiles(c["consumer"]["K0"]) == TO and vc.tiles(c["consumer"]["O"]) == TI
        # what is refused is refused by the restated rule, and nothing else is
        for c in cs:
            epi = "reduce" in c.get("form", "") or c["kind"] == "chain"
            want = None if not epi else (vc.NEEDS_O4 if c["O"] % 4 else None if vc.tile_epilogue(TI, TO, c["O"]) else vc.NO_EPILOGUE)
            assert c["refused"] == want, c
            if c["refused"] == vc.NO_EPILOGUE:
                assert (TI, TO) == (1, 1)
        for c in rows:
            hidden_by_form[(c["H"], c["form"])] += 1
            forms_by_ti[(TI, c["form"])] += 1
            if "reduce" in c["form"] and not c["refused"]:
                segs[(c["form"], c["seg_rows"], c["ragged"])] += 1
            if "group" in c["form"]:
                gpaths[(vc.group_path(c["H"], c["group_rows"]), c["H"], c["group_rows"])] += 1
    assert {vc.tiles(h) for h in vc.HIDDEN} == {1, 2, 7, 10} and set(vc.HIDDEN) == {7, 64, 200, 305, 320}
    for H in vc.HIDDEN:  # every hidden width under every form, every form at every TI
        for form in vc.FORMS:
            assert hidden_by_form[(H, form)] > 0, (H, form)
    for TI in range(1, 8):
        for form in vc.FORMS:
            assert forms_by_ti[(TI, form)] > 0, (TI, form)
    # the group term: parked in LDS and loaded per lane, every group size; and a hidden layer too wide for a parked row
    # under groups that would otherwise be parked
    assert {(p, r) for p, h, r in gpaths} >= {("lds", 18), ("lds", 32), ("lane", 5), ("lane", 18), ("lane", 32)}
    assert any(h == 320 and r >= 16 for p, h, r in gpaths) and any(p == "lds" and h == 200 for p, h, r in gpaths)
    for form in ("plain1+reduce_y", "reduce_noy"):  # the row-group sums: every group size, ragged and whole groups
        for R in vc.SEG_ROWS:
            assert segs[(form, R, True)] and segs[(form, R, False)], (form, R)
    consumers = Counter((c["consumer"]["form"], vc.tiles(c["consumer"]["K0"]), vc.tiles(c["consumer"]["O"]))
                        for cs in cases.values() for c in cs if c["kind"] == "chain")
    for TI, TO in LATTICE:
        assert consumers[("group+tail", TI, TO)] and consumers[("weighted_sums", TI, TO)], (TI, TO)


def _block_launches(cs, kind):
    n = 0
    for c in cs:
        if c["kind"] != kind:
            continue
        if kind == "rows":
            n += len(c["Ms"]) * (2 if "reduce" in c["form"] else 1)
        else:
            n += len(c["Ms"]) * (2 + (1 if c["consumer"]["form"] == "group+tail" else 2))
    return n


def test_no_test_of_part_1_is_long():
    for p, cs in _all().items():
        assert _block_launches(cs, "rows") <= 100 and _block_launches(cs, "chain") <= 100, p


def test_part_2_hits_both_float32_forms_and_every_t2():
    assert [c["T2"] for c in vc.F32_MANY] == list(range(1, 8)) and all(c["form"] == "rows" and c["M"] == vc.F32_TILE_ROWS + 1 for c in vc.F32_MANY)
    assert all(c["form"] == "tile" for c in vc.F32_FEW) and {c["T2"] for c in vc.F32_FEW} == set(range(1, 8))
    assert [c["K0"] for c in vc.F32_FEW] == [k for TI in (1, 3, 7) for k in vc.k0_edges(TI)]
    for table in (vc.F32_FEW, vc.F32_MANY):
        assert {c["H"] for c in table} == {7, 200, 320}
        assert {vc.tiles(c["K0"]) for c in table} == {1, 3, 7} and {c["K0"] % 4 == 0 for c in table} == {True, False}
        assert {bool(c["group_rows"]) for c in table} == {True, False} and {c["tail"] for c in table} == {True, False}
        assert {c["O"] % 4 == 0 for c in table} == {True, False}
        for c in table:
            assert vc.tiles(c["O"]) == c["T2"] and c["O"] in (32 * c["T2"], 32 * c["T2"] - 28, 32 * c["T2"] - 3)


def _branches():
    first = {s: vc.stream_branch(*s, frag_in=False, group=False, tail=False, partial=True, y=False, frag_out=True) for s in vc.STREAM_FIRST}
    general = {s: vc.stream_branch(*s, frag_in=False, group=False, tail=False, partial=True, y=False, frag_out=True) for s in vc.STREAM_FIRST_GENERAL}
    att = {s: vc.stream_branch(*s, frag_in=True, group=True, tail=True, partial=False, y=True, frag_out=False) for s in vc.STREAM_ATTENTION}
    feat = {s: vc.stream_branch(*s, frag_in=True, group=False, tail=False, partial=True, y=False, frag_out=False) for s in vc.STREAM_FEATURE}
    return first, general, att, feat


def test_part_3_hits_every_streamed_branch():
    first, general, att, feat = _branches()
    assert set(first.values()) == {("first", 0, 0), ("first", 0, 1)}
    assert {s[0] for s in first} == {17, 20, 29, 31, 32} and {s[1] for s in first} == {289, 304, 305, 320} and {s[2] for s in first} == {196, 200, 224}
    assert set(general.values()) == {None} and {s[0] for s in general} == {13, 16}
    assert {b for b in att.values() if b} == {("attention", i, h) for i in (0, 1) for h in (0, 1)}
    assert {(K0, H) for K0, H, O in att} >= {(i, h) for i in (208, 209) for h in (208, 209)}
    assert att[(208, 209, 200)] is None  # a hidden width that is no multiple of 4: the selector's own way to the general kernel
    assert set(feat.values()) == {("feature", i, h) for i in (0, 1) for h in (0, 1)}
    assert {(K0, H) for K0, H, O in feat} == {(i, h) for i in (208, 209) for h in (208, 209)}


def _network_blocks(dims, T, self_state_dim=6):
    """(K0, H, O) of the blocks SarlValueNet._block_specs makes of a network: mlp1, mlp2, attention (the h1 half of layer
    0 + layer 1), mlp3[:2], mlp3[2:4]."""
    h1 = dims["mlp1"][1]
    return [(T, dims["mlp1"][0], h1), (h1, dims["mlp2"][0], dims["mlp2"][1]), (h1, dims["attention"][0], dims["attention"][1]),
            (self_state_dim + dims["mlp2"][1], dims["mlp3"][0], dims["mlp3"][1]), (dims["mlp3"][1], dims["mlp3"][2], dims["mlp3"][3])]


def test_part_4_holds_the_networks_it_names():
    by = {n[0]: n for n in vc.NETWORKS}
    assert {n[2] for n in vc.NETWORKS if n[1] is vc.EBCADRL} >= {17, 29, 33, 44, 61, 65, 92, 209, 224}
    assert {n[2] for n in vc.NETWORKS if n[1] is vc.CROWDNAV} == {13, 61}
    assert set(vc.NETWORK_ROWS) == {5, 16, 18, 32, 33}
    # OM-SARL's mlp1: every input tile count against ten hidden and seven output tiles
    assert {vc.tiles(n[2]) for n in vc.NETWORKS if n[1] is vc.EBCADRL} == set(range(1, 8))
    small = _network_blocks(vc.SMALL, 13)
    assert (vc.tiles(small[0][0]), vc.tiles(small[0][2])) == (1, 1) and not vc.tile_epilogue(1, 1, small[0][2])
    assert all(h <= vc.MAX_HIDDEN for _, h, _ in small) and by["small_T13"][3:] == (1, 1)
    wide = _network_blocks(vc.WIDE_HIDDEN, 13)
    assert wide[0][1] == 512 > vc.MAX_HIDDEN and by["hidden512_T13"][3:] == (0, 0)
    for name, dims, T, native, exact in vc.NETWORKS:
        blocks = _network_blocks(dims, T)
        fits = all(k <= vc.MAX_IN and h <= vc.MAX_HIDDEN and o <= vc.MAX_OUT for k, h, o in blocks[:3])
        assert native == int(fits), name
        # the float32 form of the whole network: five blocks, and outputs the pair kernels take (multiples of 4)
        assert exact == int(fits and blocks[0][2] % 4 == 0 and blocks[1][2] % 4 == 0), name


def test_the_float64_references_are_torch_float64_linears():
    lin = torch.nn.functional.linear
    for K0, H, O, tail, R, relu in ((17, 300, 200, False, 0, 1), (209, 64, 93, False, 5, 0), (96, 305, 128, True, 18, 0)):
        w, rs = vc.make_block(K0, H, O, tail)
        M = 77
        x = rs.randn(M, K0).astype(np.float32)
        rb = rs.randn(-(-M // R), H).astype(np.float32) if R else None
        t = {k: torch.from_numpy(v).double() for k, v in w.items()}
        h = lin(torch.from_numpy(x).double(), t["w1"], t["b1"])
        if rb is not None:
            h = h + torch.from_numpy(rb).double().repeat_interleave(R, 0)[:M]
        y = lin(torch.relu(h), t["w2"], t["b2"])
        y = lin(torch.relu(y), t["w3"][None, :], t["b3"]).squeeze(1) if tail else (torch.relu(y) if relu else y)
        got = vc.mlp2_ref(x, w, relu, rb, R)
        assert got.dtype == np.float64 and got.shape == tuple(y.shape)
        np.testing.assert_allclose(got, y.numpy(), rtol=1e-12, atol=1e-13)
    # the pair sums by an explicit loop: ragged counts, weights, a last pair that M cuts short
    rs = np.random.RandomState(3)
    rows, wt, nv = rs.randn(40, 8), rs.rand(54), np.array([18, 3, 7])
    for weight, n_valid, mean in ((None, nv, True), (wt, None, False), (None, None, True)):
        got = vc.pair_sums_ref(rows, 18, 40, n_valid, weight, mean)
        for b in range(3):
            acc = np.zeros(8)
            for r in range(18 if n_valid is None else n_valid[b]):
                if b * 18 + r < 40:
                    acc += rows[b * 18 + r] * (1.0 if weight is None else wt[b * 18 + r])
            np.testing.assert_allclose(got[b], acc / ((18 if n_valid is None else n_valid[b]) if mean else 1), rtol=1e-13, atol=1e-15)


def test_the_host_split_is_the_hand_off_layout():
    """frag_pack against the layout ebc_value_net.h states (element j of lane half h in k-step s is column
    16 s + 8 (j >> 2) + 4 h + (j & 3); row = lane & 31), hi = bf16(v) and lo = bf16(v - hi); frag_unpack inverts it."""
    rs = np.random.RandomState(4)
    M, W = 45, 41
    x = rs.randn(M, W).astype(np.float32)
    f = vc.frag_pack(x)
    assert tuple(f.shape) == (2, 2, 2, 2, 64, 4) and f.dtype == torch.int32
    b = f.view(torch.bfloat16).float().numpy()  # [tile][column tile][k-step][hi, lo][lane][8]
    hi = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    lo = torch.from_numpy(x - hi).to(torch.bfloat16).float().numpy()
    for (t, c, s, lane, j) in ((0, 0, 0, 0, 0), (1, 1, 1, 37, 5), (0, 1, 0, 63, 7), (1, 0, 1, 12, 4), (0, 0, 1, 33, 3)):
        r, k = t * 32 + (lane & 31), c * 32 + 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)
        inside = r < M and k < W
        assert b[t, c, s, 0, lane, j] == (hi[r, k] if inside else 0) and b[t, c, s, 1, lane, j] == (lo[r, k] if inside else 0)
    back = vc.frag_unpack(b[:, :, :, 0] + b[:, :, :, 1], M, W)
    np.testing.assert_array_equal(back, hi + lo)
    assert float(np.abs(back - x).max()) <= 2.0 ** -16 * float(np.abs(x).max())


def test_write_the_coverage_table():
    """The counts into profiles/value_net_shape_coverage.txt; written only when it differs, so a run on an unchanged tree
    leaves the tree unchanged."""
    lines = ["# generated by tests/test_value_net_shapes_cpu.py from tests/value_net_cases.py: what",
             "# tests/test_value_net_shapes_gpu.py launches.  One row per (TI, TO) of mlp2_split_wg_kernel: the layout and waves",
             "# the selector picks, block launches without / with the group term, with KIN = 0 / 1, by input path (scalar",
             "# loads per lane / rows parked in LDS / fragments; '-': the kernel has no such path there), and forms refused.",
             "TI TO layout NW  plain group  kin0 kin1  lane  lds frag  refused"]
    total = Counter()
    everywhere = [im for p in LATTICE for im in vc.launches(*p)]
    for TI, TO in LATTICE:
        cs = vc.block_cases(TI, TO)
        n = Counter()
        for i, m in everywhere:
            if (i[0], i[1]) != (TI, TO):
                continue
            n["group" if i[3] else "plain"] += m
            n["kin%d" % i[5]] += m
            n[i[6]] += m
        cls, NW = vc.layout(TI, TO)
        has_lds = vc.input_path(TI, TO, 32 * TI) == "lds"
        refused = sum(1 for c in cs if c["refused"]) + sum(1 for c in cs if c["kind"] == "chain" and c["consumer"]["refused"])
        lines.append("%2d %2d %-6s %2d  %5d %5d  %4d %4s  %4d %4s %4d  %7d" % (
            TI, TO, cls, NW, n["plain"], n["group"], n["kin0"], n["kin1"] if TI == 7 else "-", n["lane"],
            n["lds"] if has_lds else "-", n["frag"], refused))
        total.update(n)
    lines.append("block launches of part 1: %d (%d with the group term; %d rows per lane, %d rows through LDS, %d fragments)" % (
        total["plain"] + total["group"], total["group"], total["lane"], total["lds"], total["frag"]))
    lines.append("float32 forms: %d cases on few rows (x %d row counts), %d on %d rows, T2 = %s" % (
        len(vc.F32_FEW), 1 + len(vc.F32_FEW_TAILS), len(vc.F32_MANY), vc.F32_TILE_ROWS + 1, sorted(c["T2"] for c in vc.F32_MANY)))
    first, general, att, feat = _branches()
    for name, table in (("first block", first), ("first block, K0 <= 16", general), ("attention block", att), ("feature block", feat)):
        count = Counter("general kernel" if b is None else "streamed KIN %d KH %d" % b[1:] for b in table.values())
        lines.append("%s: %s" % (name, ", ".join("%s x %d" % kv for kv in sorted(count.items()))))
    lines.append("whole networks: %d x pair sizes %s" % (len(vc.NETWORKS), list(vc.NETWORK_ROWS)))
    text = "\n".join(lines) + "\n"
    old = open(TABLE).read() if os.path.exists(TABLE) else None
    if text != old:
        with open(TABLE, "w") as f:
            f.write(text)
