"""Case tables and float64 references for the two-layer value-network blocks (csrc/ebc_value_net.h, csrc/ebc_vn_stream.h)
over the whole lattice of shapes they are compiled for.  No GPU here: tests/test_value_net_shapes_gpu.py runs the
tables on the device, tests/test_value_net_shapes_cpu.py asserts from the tables alone (and from the restatement of the
selector below) that they reach every instantiation, layout, input path and selector branch they are meant to."""
import numpy as np

# ---- the selector, restated -----------------------------------------------------------------------------------------
XROW = 144                 # ebc_vn_layout.h:10  EBC_VN_XROW
VN_GROUPS = 4              # ebc_vn_layout.h:11  EBC_VN_GROUPS
VN_GROUP_PITCH = 912       # ebc_vn_layout.h:12  EBC_VN_GROUP_PITCH
F32_TILE_ROWS = 1 << 16    # ebc_value_net.h:567 EBC_F32_TILE_ROWS
MAX_IN, MAX_HIDDEN, MAX_OUT = 224, 320, 224  # ebcsim_value_net.hip:179 (ebc_mlp2_create_ex)


def tiles(n):
    """pack_layer, ebcsim_value_net.hip:48: a dimension in tiles of 32."""
    return (n + 31) // 32


def layout(TI, TO):
    """VnLayout::lean / nw, ebc_vn_layout.h:30-33 -> (class, NW): "lean" (4 waves) where the full layout does not fit
    half a CU's LDS and the lean one does; else the full layout, with 8 waves ("full8") where it is over 80 KB."""
    full, lean, half_cu = 2 * (TI + TO) * 4096, (2 * TI + TO) * 4096, 78 * 1024
    if full > half_cu and lean <= half_cu:
        return "lean", 4
    return ("full8", 8) if full > 80 * 1024 else ("full", 4)


def kin(TI, K0):
    """launch_mlp2_to, ebcsim_value_net.hip:129-133: the last input tile's second k-step left out."""
    return int(TI == 7 and K0 <= 32 * TI - 16)


def input_path(TI, TO, K0, frag_in=False):
    """mlp2_split_wg_kernel, ebc_value_net.h:98-158: "frag" (the hand-off tensor), "lds" (rows parked in a wave's LDS tile:
    VnLayout::rows_through_lds, ebc_vn_layout.h:55 — TI >= 2, 16-byte rows, and xcap, :42, holds NW tiles of 32 x XROW bytes)
    or "lane" (scalar loads)."""
    if frag_in:
        return "frag"
    cls, NW = layout(TI, TO)
    xcap = TI * 4096 if cls == "lean" else (TI + TO) * 4096
    return "lds" if TI >= 2 and K0 % 4 == 0 and NW * 32 * XROW <= xcap else "lane"


def tile_epilogue(TI, TO, O):
    """VnLayout::has_tile_epilogue, ebc_vn_layout.h:57 (launch_mlp2_to, ebcsim_value_net.hip:126-128 / ebc_value_net.h:315):
    the coalesced epilogue (partial sums, fragments out) exists where O is a multiple of 4 and the weight region holds NW
    parked tiles."""
    cls, NW = layout(TI, TO)
    region = (2 * TI + TO) * 4096 if cls == "lean" else (TI + TO) * 8192
    return O % 4 == 0 and NW * 32 * XROW <= region


def group_path(H, group_rows):
    """ebc_value_net.h:164-171: the group terms wait in LDS when H is a multiple of 4, a wave's 32 rows meet at most
    EBC_VN_GROUPS groups and a parked row holds H floats (H <= 224); else each lane loads its own."""
    return "lds" if H % 4 == 0 and 31 // group_rows + 2 <= VN_GROUPS and H * 4 + 16 <= VN_GROUP_PITCH else "lane"


def stream_branch(K0, H, O, frag_in, group, tail, partial, y, frag_out, seg_rows=18, group_rows=18):
    """vn_stream_launch, ebcsim_vn_stream.hip:45-64 -> None (the general kernel) or (name, KIN, KH)."""
    ti, th, to = tiles(K0), tiles(H), tiles(O)
    if (not frag_in and ti == 1 and K0 > 16 and th == 10 and to == 7 and not group and not tail and partial and not y
            and seg_rows >= 16 and O % 4 == 0):
        return ("first", 0, int(H <= 32 * 10 - 16))
    if not frag_in or frag_out or ti != 7 or th != 7:
        return None
    k = (int(K0 <= 32 * 7 - 16), int(H <= 32 * 7 - 16))
    if group and tail and not partial and y and to == 7:
        if H % 4 or 31 // group_rows + 2 > VN_GROUPS:
            return None
        return ("attention",) + k
    if not group and not tail and partial and not y and to == 4 and seg_rows >= 16 and O % 4 == 0:
        return ("feature",) + k
    return None


# ---- float64 references ---------------------------------------------------------------------------------------------
def make_block(K0, H, O, tail=False, seed=None):
    """Random float32 weights of scale 1 / sqrt(fan_in), seeded as tests/test_value_net.py seeds them."""
    rs = np.random.RandomState(K0 * 1000 + H if seed is None else seed)
    w = {"w1": (rs.randn(H, K0) / np.sqrt(K0)).astype(np.float32), "b1": (rs.randn(H) * 0.1).astype(np.float32),
         "w2": (rs.randn(O, H) / np.sqrt(H)).astype(np.float32), "b2": (rs.randn(O) * 0.1).astype(np.float32)}
    if tail:
        w["w3"] = (rs.randn(O) / np.sqrt(O)).astype(np.float32)
        w["b3"] = np.array([0.3], np.float32)
    return w, rs


def mlp2_ref(x, w, relu_out, row_bias=None, group_rows=0):
    """The block on rows x in float64: relu(x W1' + b1 [+ the row's group term]) W2' + b2, then ReLU when relu_out, or the
    one-output tail w3 . relu(.) + b3 (which rectifies whatever relu_out says: ebc_value_net.h:302-313)."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    h = f(x) @ f(w["w1"]).T + f(w["b1"])
    if row_bias is not None:
        h = h + np.repeat(f(row_bias), group_rows, axis=0)[:len(h)]
    y = np.maximum(h, 0) @ f(w["w2"]).T + f(w["b2"])
    if "w3" in w:
        return np.maximum(y, 0) @ f(w["w3"]) + float(w["b3"][0])
    return np.maximum(y, 0) if relu_out else y


def pair_sums_ref(rows, R, M, n_valid=None, weight=None, mean=True):
    """ebc_pair_combine's answer in float64 from the rows themselves: per pair of R rows, the sum of its first n_valid
    rows that lie below M (times their weights), divided by n_valid (None: R) when mean."""
    B = -(-M // R)
    pad = np.zeros((B * R, rows.shape[1]))
    pad[:M] = rows[:M]
    wt = np.ones(B * R) if weight is None else np.asarray(weight, np.float64)[:B * R].copy()
    wt[M:] = 0
    wt = wt.reshape(B, R)
    if n_valid is not None:
        wt = wt * (np.arange(R)[None, :] < np.asarray(n_valid)[:, None])
    s = (pad.reshape(B, R, -1) * wt[:, :, None]).sum(1)
    if mean:
        s = s / (np.full(B, float(R)) if n_valid is None else np.asarray(n_valid, np.float64))[:, None]
    return s


def _frag_cols():
    """Column of a 32-wide tile held by (k-step s, lane, element j) of a hand-off fragment: accumulator order,
    16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3) (ebc_value_net.h:10-16, pack_layer's acc_order)."""
    s, lane, j = np.meshgrid(np.arange(2), np.arange(64), np.arange(8), indexing="ij")
    return 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3), lane & 31


def frag_unpack(frag_f32, M, width):
    """A fragment tensor read as float32 [row tiles][column tiles][2][64][8] (hi + lo already added) -> rows [M][width]."""
    col, row = _frag_cols()
    nt, ct = frag_f32.shape[:2]
    out = np.zeros((nt * 32, ct * 32), dtype=frag_f32.dtype)
    for t in range(nt):
        for c in range(ct):
            out[t * 32 + row, c * 32 + col] = frag_f32[t, c]
    return out[:M, :width]


def frag_pack(x):
    """Rows [M][width] float32 -> the hand-off tensor [row tiles][column tiles][2][2][64][4] int32 a block leaves with
    frag_out: every value split in hi = bf16(v), lo = bf16(v - hi) (round to nearest even), zeros past M and the width."""
    import torch
    M, width = x.shape
    nt, ct = tiles(M), tiles(width)
    pad = np.zeros((nt * 32, ct * 32), np.float32)
    pad[:M, :width] = x
    col, row = _frag_cols()
    v = torch.from_numpy(np.stack([[pad[t * 32 + row, c * 32 + col] for c in range(ct)] for t in range(nt)]))  # [nt][ct][2][64][8]
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo], dim=3).contiguous().view(torch.int32)  # [nt][ct][2][2][64][4]


# ---- part 1: the general block over its lattice ------------------------------------------------------------------------
HIDDEN = (7, 64, 200, 305, 320)   # not a multiple of 4, an exact tile, 7 tiles, both sides of 32 * 10 - 16
GROUP_ROWS = (5, 18, 32)
SEG_ROWS = (16, 18, 32)
FORMS = ("plain0", "plain1+reduce_y", "group", "tail", "reduce_noy", "group+tail")
NO_EPILOGUE = "no tile epilogue"  # the refusal of a block of 1 + 1 tiles (ebcsim_value_net.hip:128)
NEEDS_O4 = "multiple of 4"        # the refusal of the epilogues for an odd O (ebcsim_value_net.hip:299, :317)


def k0_edges(TI):
    """Input widths at the edges of tile TI and of its two k-steps."""
    return sorted({max(1, k) for k in (32 * (TI - 1) + 1, 32 * TI - 17, 32 * TI - 16, 32 * TI - 15, 32 * TI - 1, 32 * TI)})


def row_counts(NW):
    """One row, both sides of a tile, exactly one workgroup, two workgroups and a row: a third whose last waves lie past
    the rows."""
    return (1, 31, 33, 32 * NW, 32 * NW * 2 + 1)


def block_cases(TI, TO):
    """The cases of one (TI, TO) pair: every K0 of k0_edges(TI) with one form each, the forms rotating with TI + TO so that
    over the lattice every form meets every edge; an odd O on the plain store; a refusal of the epilogues for that odd O;
    and the hand-off chain (`mlp1` form -> fragment consumers of the transposed pair (TO, TI)).  Group forms sit three
    places apart: one on either side of the KIN boundary at TI = 7."""
    NW = layout(TI, TO)[1]
    Ms = row_counts(NW)
    rot = TI + TO
    cases = []
    for j, K0 in enumerate(k0_edges(TI)):
        f = (j + rot) % 6
        form, var = FORMS[f], TI + 2 * TO + f // 3  # var: what the two group forms / the two reduce forms of a pair differ in
        H = HIDDEN[(j + 2 * rot) % 5]
        alt = (j + rot // 2) % 2  # decoupled from the form's parity: over the lattice every form meets either value
        O = 32 * TO if alt else 32 * (TO - 1) + 4
        c = dict(kind="rows", K0=K0, H=H, O=O, form=form, relu=alt, group_rows=GROUP_ROWS[var % 3],
                 seg_rows=SEG_ROWS[var % 3], ragged=bool(var % 2), Ms=Ms, refused=None)
        if "reduce" in form:
            c["relu"] = 1 if "plain1" in form else c["relu"]
            if not tile_epilogue(TI, TO, O):
                c["refused"] = NO_EPILOGUE
        cases.append(c)
    # the attention stack's form at the widest input of the pair: the group terms parked in LDS beside rows parked in LDS
    cases.append(dict(kind="rows", K0=32 * TI, H=200, O=32 * TO, form="group+tail" if rot % 2 else "group", relu=rot % 2,
                      group_rows=18, seg_rows=0, ragged=False, Ms=Ms, refused=None))
    K0 = k0_edges(TI)[rot % 6]
    cases.append(dict(kind="rows", K0=K0, H=HIDDEN[rot % 5], O=32 * TO - 3, form="plain%d" % (rot % 2), relu=rot % 2,
                      group_rows=0, seg_rows=0, ragged=False, Ms=Ms, refused=None))
    cases.append(dict(kind="rows", K0=K0, H=HIDDEN[rot % 5], O=32 * TO - 3, form="reduce_noy", relu=1, group_rows=0,
                      seg_rows=18, ragged=False, Ms=(33,), refused=NEEDS_O4))
    # the hand-off chain.  Producer (TI, TO): rows in, fragments + partial sums out, no rows (SarlValueNet's `mlp1`); its
    # output is as wide as a consumer's input on either side of that tile's k-step boundary.  Consumers: the pair (TO, TI)
    # with fragment input, as the attention stack (group + tail) and as `mlp2` (weighted partial sums, no rows).
    NWc = layout(TO, TI)[1]
    Mc = tuple(sorted(set(Ms) | set(row_counts(NWc))))
    for n, (K0, width) in enumerate(((32 * TI - 15, 32 * TO), (32 * TI - 16, 32 * TO - 16))):
        cases.append(dict(kind="chain", K0=K0, H=HIDDEN[(n + rot) % 5], O=width, seg_rows=SEG_ROWS[(n + rot) % 3],
                          refused=None if tile_epilogue(TI, TO, width) else NO_EPILOGUE, Ms=Mc,
                          consumer=dict(K0=width, H=HIDDEN[(n + 2 + rot) % 5], O=32 * TI if n else 32 * (TI - 1) + 4,
                                        form="group+tail" if (n + rot) % 2 else "weighted_sums",
                                        group_rows=GROUP_ROWS[(n + rot) % 3],
                                        refused=None if (n + rot) % 2 or tile_epilogue(TO, TI, 32 * TI) else NO_EPILOGUE)))
    for c in cases:
        assert c["K0"] <= MAX_IN and c["H"] <= MAX_HIDDEN and c["O"] <= MAX_OUT and tiles(c["K0"]) == TI and tiles(c["O"]) == TO
    return cases


def launches(TI, TO):
    """((TI, TO, NW, GROUP, layout, KIN, input path), block launches) of every case of block_cases(TI, TO) that is not
    refused; a chain's consumer is an instantiation of the transposed pair."""
    out = []
    cls, NW = layout(TI, TO)
    for c in block_cases(TI, TO):
        me = (TI, TO, NW, "group" in c.get("form", ""), cls, kin(TI, c["K0"]), input_path(TI, TO, c["K0"]))
        if c["kind"] == "rows":
            if c["refused"] != NEEDS_O4:  # (a refused reduce form still has its plain rows beside it)
                out.append((me, len(c["Ms"]) * (2 if "reduce" in c["form"] and not c["refused"] else 1)))
        else:
            out.append((me, len(c["Ms"]) * (1 if c["refused"] else 2)))  # the plain rows and the `mlp1` form
            d = c["consumer"]
            clc, NWc = layout(TO, TI)
            if not d["refused"]:
                out.append(((TO, TI, NWc, "group" in d["form"], clc, kin(TO, d["K0"]), "frag"),
                            len(c["Ms"]) * (1 if "group" in d["form"] else 2)))
    return out


def instantiations(TI, TO):
    return [i for i, _ in launches(TI, TO)]


# ---- part 2: the float32 forms ---------------------------------------------------------------------------------------------
F32_HIDDEN = (7, 200, 320)
F32_K0 = tuple(k for TI in (1, 3, 7) for k in k0_edges(TI))


def _f32_case(i, K0, T2, M):
    O = (32 * T2, 32 * (T2 - 1) + 4, 32 * T2 - 3)[i % 3]
    return dict(K0=K0, H=F32_HIDDEN[(i // 3) % 3], O=O, T2=T2, group_rows=18 if i % 2 else 0, tail=bool((i // 2) % 2),
                relu=(i // 4) % 2, M=M,
                form="tile" if M <= F32_TILE_ROWS else "rows")


# few rows (a workgroup per tile): every K0, the output tiles rotating; the tails of the batch are taken from its first rows
F32_FEW = tuple(_f32_case(i, K0, 1 + i % 7, 18 * 7 + 5) for i, K0 in enumerate(F32_K0))
F32_FEW_TAILS = (1, 31, 33)
# many rows (mlp2_f32_kernel<T2>): the smallest count above EBC_F32_TILE_ROWS, every T2, K0 walking the list in steps of 5
F32_MANY = tuple(_f32_case(t, F32_K0[(5 * t + 2) % len(F32_K0)], 1 + t, F32_TILE_ROWS + 1) for t in range(7))


# ---- part 3: the streamed kernels ----------------------------------------------------------------------------------------------
STREAM_FIRST = tuple((K0, H, O) for K0 in (17, 20, 29, 31, 32) for H in (289, 304, 305, 320) for O in (196, 200, 224))
STREAM_FIRST_GENERAL = ((16, 300, 200), (13, 300, 200))  # the selector's K0 > 16: these take the general kernel
STREAM_ATTENTION = tuple((K0, H, 200) for K0 in (208, 209) for H in (208, 209)) + ((208, 212, 224), (212, 208, 196), (209, 212, 200))
STREAM_FEATURE = tuple((K0, H, 100) for K0 in (208, 209) for H in (208, 209))


# ---- part 4: whole networks ----------------------------------------------------------------------------------------------------
EBCADRL = dict(mlp1=(300, 200), mlp2=(200, 100), attention=(200, 200, 1), mlp3=(300, 200, 200, 1))
CROWDNAV = dict(mlp1=(150, 100), mlp2=(100, 50), attention=(100, 100, 1), mlp3=(150, 100, 100, 1))
SMALL = dict(mlp1=(64, 32), mlp2=(32, 16), attention=(32, 32, 1), mlp3=(32, 32, 32, 1))
WIDE_HIDDEN = dict(mlp1=(512, 200), mlp2=(200, 100), attention=(200, 200, 1), mlp3=(300, 200, 200, 1))
NETWORK_ROWS = (5, 16, 18, 32, 33)
# (name, dims, T, forwards counted by native_forwards per coarse forward, by native_exact_forwards per exact one)
NETWORKS = tuple(("ebcadrl_T%d" % T, EBCADRL, T, 1, 1) for T in (17, 29, 33, 44, 61, 65, 92, 113, 157, 182, 209, 224)) + (
    # mlp2 has 50 outputs: the blocks run, the pair kernels of the float32 form do not take it (torch's float32 GEMMs)
    ("crowdnav_T13", CROWDNAV, 13, 1, 0), ("crowdnav_T61", CROWDNAV, 61, 1, 0),
    # mlp1 and mlp2 are blocks of 1 + 1 tiles: no tile epilogue, so the pair sums are not folded into them
    ("small_T13", SMALL, 13, 1, 1),
    # a hidden layer wider than ebc_mlp2_create_ex takes: torch for the whole network, and the counters say so
    ("hidden512_T13", WIDE_HIDDEN, 13, 0, 0))


def network_state_dict(dims, T, seed, self_state_dim=6):
    """A random-init state_dict of the reference's ValueNetwork layout (mlp1 / mlp2 / attention / mlp3 as Sequentials of
    Linear + ReLU: the Linear layers sit at the even indices), torch's default Linear init, float32."""
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def stack(prefix, fan_in, widths):
        for i, o in enumerate(widths):
            bound = 1.0 / fan_in ** 0.5
            sd["%s.%d.weight" % (prefix, 2 * i)] = (torch.rand(o, fan_in, generator=g) * 2 - 1) * bound
            sd["%s.%d.bias" % (prefix, 2 * i)] = (torch.rand(o, generator=g) * 2 - 1) * bound
            fan_in = o
    stack("mlp1", T, dims["mlp1"])
    stack("mlp2", dims["mlp1"][-1], dims["mlp2"])
    stack("attention", 2 * dims["mlp1"][-1], dims["attention"])
    stack("mlp3", self_state_dim + dims["mlp2"][-1], dims["mlp3"])
    return sd
