"""Cases of the wide two-layer value-network block (ebc_mlp2_create_wide, csrc/ebc_vn_wide.h) and of the networks that
decide with it (SarlValueNet(..., wide=True)): shapes, row counts and the networks' stacks, shared by
tests/test_vn_wide_cpu.py and tests/test_vn_wide_gpu.py.  Weights, inputs and float64 references are those of
tests/value_net_cases.py (make_block / mlp2_ref: randn / sqrt(fan_in), inputs 2 * randn)."""

LIMIT = 640                # EBC_VNW_MAX, ebc_vn_wide.h
ROWS_PER_WORKGROUP = 256   # EBC_VNW_ROWS, ebc_vn_wide.h (ebcsim.mlp2.Mlp2Block.WIDE_ROWS_PER_WORKGROUP)

# each dimension just past the narrow block's limit (225, 321, 225) and at the wide one's (640); widths that are no
# multiple of 4 or 32; one wide dimension beside narrow ones; a narrow shape on the wide entry
BLOCK_SHAPES = ((17, 600, 400), (400, 400, 200), (206, 600, 400), (300, 300, 1), (225, 321, 225), (257, 352, 640),
                (640, 640, 640), (230, 333, 227), (13, 512, 200), (5, 7, 3))
ROW_COUNTS = (1, 31, 33, 515)
# waves and workgroups past the last row tile: three workgroups and one row, one row less than a workgroup, 18
EDGE_SHAPE = (400, 400, 200)
EDGE_ROW_COUNTS = (32 * (ROWS_PER_WORKGROUP // 32) * 3 + 1, ROWS_PER_WORKGROUP - 1, 18)
# (K0, H, O), R, B: the attention form (group term + one-output tail); M = B * R is no multiple of 32, and at R = 18 a
# 32-row tile meets three groups (rows 32 .. 63: groups 1, 2, 3)
ATTENTION_CASES = (((400, 400, 400), 1, 77), ((400, 400, 400), 5, 103), ((400, 400, 400), 18, 29), ((400, 400, 400), 33, 17),
                   ((230, 333, 227), 7, 75), ((640, 640, 640), 5, 103))
# shapes both entries take: (K0, H, O), group rows (0: none), tail
SHARED_SHAPES = (((200, 200, 200), 18, True), ((17, 300, 200), 0, False), ((224, 320, 224), 0, False))
F32_ROW_COUNTS = (1, 33, 515)
REPACK_SHAPES = (((400, 400, 400), True), ((17, 600, 400), False))

X2 = dict(mlp1=(300, 200), mlp2=(200, 100), attention=(200, 200, 1), mlp3=(300, 200, 200, 1))  # policy_x2.config
X3 = dict(mlp1=(400, 300), mlp2=(300, 100), attention=(300, 300, 1), mlp3=(400, 300, 300, 1))  # policy_x3.config
X4 = dict(mlp1=(600, 400), mlp2=(400, 200), attention=(400, 400, 1), mlp3=(600, 400, 400, 1))
HIDDEN512 = dict(mlp1=(512, 200), mlp2=(200, 100), attention=(200, 200, 1), mlp3=(300, 200, 200, 1))  # value_net_cases.WIDE_HIDDEN
TOO_WIDE = dict(mlp1=(700, 200), mlp2=(200, 100), attention=(200, 200, 1), mlp3=(300, 200, 200, 1))

N, W = "narrow", "wide"
# name -> (dims, T, plan_blocks(...) with wide False, with wide True): ([mlp1, mlp2, attention, mlp3[:2], mlp3[2:4]], gterm)
PLANS = {
    "x2": (X2, 17, ([N] * 5, N), ([N] * 5, N)),
    "x3": (X3, 17, None, ([W] * 5, W)),
    "x4": (X4, 17, None, ([W] * 5, W)),
    "hidden512": (HIDDEN512, 13, None, ([W, N, N, N, N], N)),
    "too_wide": (TOO_WIDE, 13, None, None),
}
# (name, dims, T) of the whole networks the GPU test runs with wide=True
NETWORKS = (("x3_T17", X3, 17), ("x4_T17", X4, 17), ("x4_T65", X4, 65), ("hidden512_T13", HIDDEN512, 13), ("x2_T17", X2, 17))


def stack_shapes(dims, T, self_state_dim=6):
    """(out, in) per layer of the four stacks, as SarlValueNet reads them off its tensors."""
    def stack(fan_in, widths):
        out = []
        for o in widths:
            out.append((o, fan_in))
            fan_in = o
        return out
    return (stack(T, dims["mlp1"]), stack(dims["mlp1"][-1], dims["mlp2"]), stack(2 * dims["mlp1"][-1], dims["attention"]),
            stack(self_state_dim + dims["mlp2"][-1], dims["mlp3"]))
