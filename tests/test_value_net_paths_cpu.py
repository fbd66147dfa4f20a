"""ebcsim.sarl.select_path — which body SarlValueNet._forward runs — against a table written out by hand from the
conditions the forward had when it was one function: every network of value_net_cases.NETWORKS, every pair size of
NETWORK_ROWS, coarse and exact, with and without the attention weights, both switches, autograd and a CPU device.  No
GPU and no library: the selector takes facts, and the facts of a network are worked out here from its dims."""
import itertools

import value_net_cases as vc
from ebcsim.sarl import PATHS, PathFacts, select_path

ROWS = vc.NETWORK_ROWS  # (5, 16, 18, 32, 33): below, at both ends of and above the folded path's 16 .. 32
FOLD = ("blocks", "folded_frag", "folded_frag", "folded_frag", "blocks")
ALL = lambda name: (name,) * len(ROWS)  # noqa: E731
# rows: (exact, want_weights) -> the path at every R of ROWS, frag_handoff and native_exact on, inference on the device
TABLE = {
    # every stack a block, mlp1 and mlp2 with the tile epilogue, widths the pair kernels take
    "ebcadrl, T <= 32": {(False, False): FOLD, (False, True): ALL("blocks"),
                         (True, False): ALL("exact_native"), (True, True): ALL("torch")},
    # the same with rows wider than a tile: exact with the weights keeps mlp1 in the library
    "ebcadrl, T > 32": {(False, False): FOLD, (False, True): ALL("blocks"),
                        (True, False): ALL("exact_native"), (True, True): ALL("exact_mlp1")},
    # mlp2 has 50 outputs: no tile epilogue (never folded), and the pair kernels of the float32 form do not take it
    "crowdnav_T13": {(False, False): ALL("blocks"), (False, True): ALL("blocks"),
                     (True, False): ALL("torch"), (True, True): ALL("torch")},
    "crowdnav_T61": {(False, False): ALL("blocks"), (False, True): ALL("blocks"),
                     (True, False): ALL("exact_mlp1"), (True, True): ALL("exact_mlp1")},
    # mlp1 and mlp2 are blocks of 1 + 1 tiles: no tile epilogue (never folded); 32 and 16 outputs suit the pair kernels
    "small_T13": {(False, False): ALL("blocks"), (False, True): ALL("blocks"),
                  (True, False): ALL("exact_native"), (True, True): ALL("torch")},
    # a hidden layer of 512: no blocks at all
    "hidden512_T13": {key: ALL("torch") for key in itertools.product((False, True), repeat=2)},
}


def _row(name, T):
    return name if name in TABLE else "ebcadrl, T <= 32" if T <= 32 else "ebcadrl, T > 32"


def _epilogue(K0, O):
    """Mlp2Block.__init__'s tile_epilogue."""
    return O % 4 == 0 and (K0 + 31) // 32 + (O + 31) // 32 >= 3


def _facts(name, dims, T):
    """PathFacts of a network on a HIP device: five blocks (mlp1, mlp2, attention, mlp3 in two), the gterm block and the
    fragment twins — all of NETWORKS but the hidden-512 one, whose mlp1 ebc_mlp2_create_ex does not take."""
    if name == "hidden512_T13":
        return PathFacts(True, 0, 0, 0, False, False, False, False)
    h1, f = dims["mlp1"][-1], dims["mlp2"][-1]
    return PathFacts(True, 5, h1, f, _epilogue(T, h1), _epilogue(h1, f), True, True)


def _paths(name, dims, T, device="cuda", frag_handoff=True, native_exact=True, grad=False):
    return {(exact, ww): tuple(select_path(_facts(name, dims, T), device, frag_handoff, native_exact, R, T, exact, ww, grad)
                               for R in ROWS)
            for exact in (False, True) for ww in (False, True)}


def test_every_network_takes_the_path_of_the_table():
    for name, dims, T, _, _ in vc.NETWORKS:
        want = TABLE[_row(name, T)]
        assert _paths(name, dims, T) == want, name
        # h1 handed on as rows: the folded path's other body, nothing else moves
        rows_form = {k: tuple("folded_rows" if p == "folded_frag" else p for p in v) for k, v in want.items()}
        assert _paths(name, dims, T, frag_handoff=False) == rows_form, name
        # without the library's float32 blocks every exact forward is torch's, and no coarse one moves
        torch_exact = {k: ALL("torch") if k[0] else v for k, v in want.items()}
        assert _paths(name, dims, T, native_exact=False) == torch_exact, name
        # autograd, and rows on the CPU: torch whatever else holds
        for kw in (dict(grad=True), dict(device="cpu")):
            assert all(v == ALL("torch") for v in _paths(name, dims, T, **kw).values()), (name, kw)
    assert {p for row in TABLE.values() for v in row.values() for p in v} | {"folded_rows"} == set(PATHS)


def test_the_counter_columns_of_the_networks_agree_with_the_paths():
    """NETWORKS' `native` counts coarse forwards on the blocks, `native_exact` exact ones in the library's float32 form."""
    for name, dims, T, native, native_exact in vc.NETWORKS:
        p = _paths(name, dims, T)
        assert all((c in ("folded_frag", "folded_rows", "blocks")) == bool(native) for c in p[(False, False)]), name
        assert all((c == "exact_native") == bool(native_exact) for c in p[(True, False)]), name


def test_small_network_is_never_folded_and_crowdnav_exact_follows_the_row_width():
    seen = 0
    for name, dims, T, _, _ in vc.NETWORKS:
        for kw in (dict(), dict(frag_handoff=False), dict(native_exact=False)):
            p = _paths(name, dims, T, **kw)
            if name == "small_T13":
                assert not any(c.startswith("folded") for v in p.values() for c in v)
                seen += 1
        if name.startswith("crowdnav"):
            p = _paths(name, dims, T)
            assert T <= 32 or T == 61
            assert p[(True, False)] == p[(True, True)] == ALL("torch" if T <= 32 else "exact_mlp1"), name
            seen += 1
    assert seen == 3 + 2
