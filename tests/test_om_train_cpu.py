"""Training OM-SARL, without a GPU: the stored state (ebcsim.occupancy.wide_state) against the reference's own
SARL.transform with with_om = true on every state of tests/golden/om_train_states.npz; the host build of the gradient rule
on wide rows (tests/native/sarl_grad_om_host.cc) against float64 autograd of the wide SarlModule, against the plain host
build at om_width = 0, and under the sanitizers; the packed image of a wide state_dict; the refusals that need no device.
Cases and the bars: tests/om_train_cases.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import om_train_cases as oc
import sarl_grad_cases as sg
from om_cases import MARGIN, compare_maps
from oracle import oracle
from ebcsim import _abi, _capi
from ebcsim.occupancy import OccupancySpec, boundary_margin, occupancy_maps, wide_state, widen
from ebcsim.sarl_train import SarlTrainer, pack_state_dict, packed_floats, shape_of, unpack_to_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")


# ---------------------------------------------------------------------- the stored state against the reference's transform
def test_wide_state_against_the_reference_transform():
    """EVERY state of the golden: the map columns of wide_state equal the recorded ones under tests/test_om_cpu.py's rule
    (occupancy equal, mean velocities within one float32 unit), the first T columns hold the 1e-5 the rotated-row tests
    apply to the numpy path (tests/test_rotated_rows_cpu.py).  A lone row: the reference's build_occupancy_maps raises on
    it (the golden then holds rotate(state) alone); the product gives it an empty map."""
    states, meta = oc.golden_states()
    assert len(states) == meta["states"] == 72 and meta["margin"] == MARGIN
    seen, lone, worst = set(), 0, 0.0
    for robot, ob, types, T, unicycle, spec, kind, want in states:
        R = len(ob)
        assert float(boundary_margin(ob[None], None, spec).min()) >= MARGIN  # none the generator should have drawn again
        rows15 = np.concatenate([np.broadcast_to(robot, (R, 9)), ob, types[:, None].astype(np.float64)], axis=1)
        rotated = oracle.rotate_rows(rows15, T == 17, unicycle)
        got = wide_state(rotated[None], ob[None], None, spec)[0]
        assert got.dtype == np.float32 and got.shape == (R, T + spec.width)
        assert got[:, :T].tobytes() == rotated.tobytes()
        np.testing.assert_allclose(got[:, :T], want[:, :T], atol=1e-5, rtol=1e-5)
        if R == 1:
            assert want.shape == (1, T) and not got[:, T:].any()
            lone += 1
        else:
            assert want.shape == (R, T + spec.width)
            worst = max(worst, compare_maps(got[:, T:], np.ascontiguousarray(want[:, T:]), spec))
        seen.add((T, spec.channels, spec.cell_num, R, kind, unicycle))
    print("72 states, %d lone rows, largest mean-velocity difference %.3g" % (lone, worst))
    assert lone == meta["one_row_raises"] == 12
    assert {s[0] for s in seen} == {13, 17} and {s[1] for s in seen} == {1, 2, 3} and {s[2] for s in seen} == {1, 4}
    assert {s[3] for s in seen} == {1, 2, 3, 4, 5, 6} and {s[4] for s in seen} == {"random", "standing", "coincident"} and {s[5] for s in seen} == {0, 1}
    # standing rows of both signs of vx are among them
    vx = np.concatenate([ob[:, 2] for _, ob, _, _, _, _, kind, _ in states if kind == "standing"])
    assert ((vx == 0) & np.signbit(vx)).any() and ((vx == 0) & ~np.signbit(vx)).any()
    # some maps are not empty, for every channel count and both grids
    filled = {(spec.channels, spec.cell_num) for _, ob, _, T, _, spec, _, want in states if len(ob) > 1 and want[:, T:].any()}
    assert filled == {(c, n) for c in (1, 2, 3) for n in (1, 4)}


def test_wide_state_is_widen_over_occupancy_maps_and_pads_with_zero_maps():
    rs = np.random.RandomState(5)
    spec = OccupancySpec(4, 1.0, 3)
    ob = rs.uniform(-2, 2, (3, 4, 5))
    rot = rs.normal(size=(3, 4, 17)).astype(np.float32)
    nv = np.array([4, 2, 0])
    ob[1, 2:] = np.nan  # rows at or past the count are never read
    got = wide_state(rot, ob, nv, spec)
    assert got.tobytes() == widen(rot[:, None], occupancy_maps(ob, nv, spec))[:, 0].tobytes()
    assert got[:, :, :17].tobytes() == rot.tobytes() and not got[1, 2:, 17:].any() and not got[2, :, 17:].any() and got[0, :, 17:].any()


# ---------------------------------------------------------------------- the rule on wide rows
@pytest.mark.parametrize("ni,B,R", oc.ACCURACY_CASES)
def test_host_build_against_float64_autograd(ni, B, R):
    """T + W = 61, 65 and 224, both values of with_global_state, ragged n_valid and a masked state: per layer and for the
    loss the rule's error against float64 autograd of the wide SarlModule is within 8 x torch's own float32 error (8 x 2^-25
    where torch's is below 2^-25).  Precondition: in float64 no score is exactly 0 and no softmax denominator is 0."""
    layers, loss, (min_score, min_den) = oc.accuracy_row(ni, B, R)
    for name, err_rule, err_t32, bar in layers + [("loss_sum",) + loss]:
        print("net %d (%s) B %d R %d %-14s rule %.3e torch32 %.3e bar %.3e%s" % (ni, oc.net_name(oc.ACCURACY_NETS[ni]), B, R, name, err_rule, err_t32, bar,
                                                                                 " (floor)" if err_t32 < oc.YARDSTICK_FLOOR else ""))
    assert min_score > 0 and min_den > 0, (min_score, min_den)
    for name, err_rule, err_t32, bar in layers + [("loss_sum",) + loss]:
        assert err_rule <= bar, (name, err_rule, err_t32, bar)


def test_accuracy_cases_cover_the_widths():
    widths = {oc.ACCURACY_NETS[ni][0][0][0] for ni, _, _ in oc.ACCURACY_CASES}
    assert widths == {61, 65, 224}
    assert {(oc.ACCURACY_NETS[ni][0][0][0], oc.ACCURACY_NETS[ni][0][2]) for ni, _, _ in oc.ACCURACY_CASES} >= {
        (w, g) for w in (65, 224) for g in (True, False)}
    assert oc.host_lib().sarl_grad_om_host_max_om() == 192 and oc.host_lib().sarl_grad_om_host_max_wide() == 224
    assert oc.host_lib().sarl_grad_om_host_max_row() == 256


@pytest.mark.parametrize("net", [sg.NARROW_NET, sg.NARROW_T17_NET, sg.NARROW_LOCAL_NET, sg.REFERENCE_NET],
                         ids=["narrow", "rows_17", "no_global_state", "reference"])
def test_om_width_zero_gives_the_bytes_of_the_plain_host_build(net):
    sd = sg.random_state_dict(net)
    P = sg.host_pack(sd)
    assert sg.same_bytes(oc.host_pack(sd, 0), P) and oc.host_floats((net, 0)) == sg.host_floats(net)
    for B, R in ((5, 3), (1, 1)):
        rows, target, nv, mask, _ = sg.edge_batch(net, B, R)
        assert oc.same_results(oc.host_grad(P, (net, 0), rows, target, nv, mask, 2.0 / B), sg.host_grad(P, net, rows, target, nv, mask, 2.0 / B))
        rows, target = sg.plain_batch(net, B, R)
        assert oc.same_results(oc.host_grad(P, (net, 0), rows, target, None, None, 0.3), sg.host_grad(P, net, rows, target, None, None, 0.3))


def test_map_columns_reach_layer_zero_alone():
    """A wide row is a longer chain in layer 0 and nothing else: with the map columns' weights at 0 the values, the loss and
    every gradient entry outside those columns are the bytes of the narrow network on the rotated columns."""
    wnet = oc.NARROW_WIDE[1]
    (widths, S, glob), W = wnet
    T = widths[0] - W
    sd = sg.random_state_dict(wnet[0])
    sd["mlp1.0.weight"][:, T:] = 0.0
    narrow = dict(sd)
    narrow["mlp1.0.weight"] = sd["mlp1.0.weight"][:, :T].clone()
    rows, target = oc.wide_batch(wnet, 5, 3, seed=91)
    nv, mask = oc.ragged_masked(5, 3, seed=92)
    wide = oc.host_grad(oc.host_pack(sd, W), wnet, rows, target, nv, mask, 0.5)
    nnet = shape_of(narrow)
    want = sg.host_grad(sg.host_pack(narrow), nnet, rows[:, :, :T], target, nv, mask, 0.5)
    assert oc.same_results((want[0][:0],) + wide[1:], (want[0][:0],) + want[1:])
    O0p = (widths[1] + 3) // 4 * 4
    g0w, g0n = wide[0][:(T + W + 1) * O0p].reshape(T + W + 1, O0p), want[0][:(T + 1) * O0p].reshape(T + 1, O0p)
    assert sg.same_bytes(g0w[:T], g0n[:T]) and sg.same_bytes(g0w[T + W], g0n[T]) and sg.same_bytes(wide[0][(T + W + 1) * O0p:], want[0][(T + 1) * O0p:])
    assert g0w[T:T + W].any()  # the map columns' own gradient is there


def test_host_program_runs_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, built with -fsanitize=address,undefined, over wide batches at T + W = 61, 65 and 224 (edge
    values in n_valid and the mask, NaN past n_valid) and at the reference widths with 65: no finding, and the bytes of the
    library build.  The program is a process of its own: nothing of it is loaded into this one."""
    batch_list = []
    for wnet, shapes in [(w, [(B, 3) for B in oc.BATCHES]) for w in oc.NARROW_WIDE] + [(oc.REFERENCE_WIDE_65, [(5, 2)]),
                                                                                          (oc.wide_net(32, 192, glob=False), [(9, 1)])]:
        P = oc.host_pack(sg.random_state_dict(wnet[0]), wnet[1])
        for B, R in shapes:
            rows, target, nv, mask, _ = sg.edge_batch(wnet[0], B, R)
            batch_list.append((wnet, P, rows, target, nv, mask, 2.0 / B))
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    oc.write_batches(src, batch_list)
    done = subprocess.run([oc.host_program(sanitize=True), src, out], check=True, capture_output=True, text=True, timeout=600)
    assert "sarl_grad_om_host: %d batches" % len(batch_list) in done.stdout and "runtime error" not in done.stderr, done.stderr
    assert "Sanitizer" not in done.stderr, done.stderr
    for (wnet, P, rows, target, nv, mask, scale), got in zip(batch_list, oc.read_results(out, batch_list)):
        assert oc.same_results(got, oc.host_grad(P, wnet, rows, target, nv, mask, scale))


# ---------------------------------------------------------------------- the packed image of a wide state_dict
@pytest.mark.parametrize("wnet", oc.NARROW_WIDE + [oc.REFERENCE_WIDE_65], ids=["61", "65", "224", "reference_65"])
def test_pack_and_unpack_of_a_wide_state_dict(wnet):
    net, W = wnet
    sd = sg.random_state_dict(net)
    assert shape_of(sd) == (list(net[0]), net[1], net[2])
    flat = pack_state_dict(sd)
    assert flat.numel() == packed_floats(*net) == oc.host_floats(wnet) and sg.same_bytes(flat.numpy(), oc.host_pack(sd, W))
    back = unpack_to_state_dict(flat, *net)
    ref = sg.module(net).state_dict()
    assert list(back) == list(ref) == list(sd)
    for k in sd:
        assert back[k].shape == ref[k].shape and torch.equal(back[k], sd[k]), k
    assert back["mlp1.0.weight"].shape[1] == net[0][0]
    sg.module(net).load_state_dict(back, strict=True)
    pad = pack_state_dict({k: torch.ones_like(v) for k, v in sd.items()}) == 0
    assert bool(pad.any()) and bool((flat[pad] == 0).all()) and (flat[pad].numpy().view(np.uint32) == 0).all()


def test_autograd_trainer_takes_wide_rows():
    """SarlTrainer(native=False, om_width=W) over a wide batch agrees with the rule's host build to float32 rounding; rows
    of another width are refused."""
    wnet = oc.NARROW_WIDE[1]
    sd = sg.random_state_dict(wnet[0])
    rows, target = oc.wide_batch(wnet, 9, 5, seed=93)
    nv, mask = oc.ragged_masked(9, 5, seed=94)
    tr = SarlTrainer(sd, device="cpu", native=False, om_width=wnet[1])
    assert tr.widths[0] == 65 and tr.om_width == 48
    loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
    live = sg.is_live(nv, mask)
    g, hl, hc, _, _ = oc.host_grad(oc.host_pack(sd, wnet[1]), wnet, rows, target, nv, mask, 2.0 / live.sum())
    assert int(count) == hc == int(live.sum()) and abs(float(loss) - hl) <= 1e-5 * hl
    np.testing.assert_allclose(tr.flat.grad.numpy(), g, rtol=0, atol=2e-5 * np.abs(g).max())
    with pytest.raises(ValueError, match="rows are 17 wide, the network takes 65"):
        tr.loss_and_grad(torch.from_numpy(rows[:, :, :17].copy()), torch.from_numpy(target))
    tr.step()
    assert list(tr.state_dict()) == list(sd) and tr.state_dict()["mlp1.0.weight"].shape == (wnet[0][0][1], 65)


# ---------------------------------------------------------------------- refusals without a device
def test_the_wide_rule_refuses_by_code():
    w = [17] + oc.NARROW_UNITS
    assert oc.host_refused(w, 6, 0) == 0 and oc.host_refused(w, 6, 48) == 0 and oc.host_refused(w, 6, 192) == 0
    assert oc.host_refused(w, 6, 193) == 14 and oc.host_refused(w, 6, -1) == 14
    assert oc.host_refused([33] + oc.NARROW_UNITS, 6, 192) == 15 and oc.host_refused([32] + oc.NARROW_UNITS, 6, 192) == 0
    assert oc.host_refused([65] + oc.NARROW_UNITS, 6, 0) == 1 and oc.host_refused([0] + oc.NARROW_UNITS, 0, 4) == 1
    assert oc.host_refused(w, 18, 48) == 13  # the self state lies inside the rotated columns


def _weights(T, units=None, self_dim=6, size=None):
    units = oc.NARROW_UNITS if units is None else units
    w = _abi.EbcSarlNetWeights()
    w.struct_size = C.sizeof(w) if size is None else size
    w.n_mlp1, w.n_mlp2, w.n_attention, w.n_mlp3 = 2, 2, 3, 4
    w.with_global_state, w.self_state_dim, w.input_dim = 1, self_dim, T
    for i, u in enumerate(units):
        w.widths[i] = u
    return w


def _refused(rc, code, *words):
    assert rc == code, (rc, _capi.lib().ebc_last_error())
    msg = _capi.lib().ebc_last_error()
    for word in words:
        assert word in msg, msg


def test_net_create_om_refuses_without_a_device():
    """om_width 193 and -1, T + W = 225, a bad struct_size, NULL arguments, T outside 1 .. 64: every one by name, before
    any weight is read or any device call is made (the weight pointers here are NULL)."""
    L = _capi.lib()
    out = C.c_void_p()
    w = _weights(17)
    _refused(L.ebc_sarl_net_create_om(C.addressof(w), 193, 0, C.byref(out)), _abi.ERR_UNSUPPORTED, b"ebc_sarl_net_create_om", b"om_width 193", b"0 .. 192")
    _refused(L.ebc_sarl_net_create_om(C.addressof(w), -1, 0, C.byref(out)), _abi.ERR_UNSUPPORTED, b"om_width -1")
    w33 = _weights(33)
    _refused(L.ebc_sarl_net_create_om(C.addressof(w33), 192, 0, C.byref(out)), _abi.ERR_UNSUPPORTED, b"T + om_width = 225", b"224")
    w65 = _weights(65)
    _refused(L.ebc_sarl_net_create_om(C.addressof(w65), 0, 0, C.byref(out)), _abi.ERR_UNSUPPORTED, b"ebc_sarl_net_create_om", b"rows of 65 floats", b"1 .. 64")
    _refused(L.ebc_sarl_net_create(C.addressof(w65), 0, C.byref(out)), _abi.ERR_UNSUPPORTED, b"ebc_sarl_net_create:", b"rows of 65 floats", b"1 .. 64")
    bad = _weights(17, size=C.sizeof(_abi.EbcSarlNetWeights) - 8)
    _refused(L.ebc_sarl_net_create_om(C.addressof(bad), 48, 0, C.byref(out)), _abi.ERR_INVALID, b"EbcSarlNetWeights.struct_size")
    _refused(L.ebc_sarl_net_create_om(None, 48, 0, C.byref(out)), _abi.ERR_INVALID, b"EbcSarlNetWeights.struct_size")
    _refused(L.ebc_sarl_net_create_om(C.addressof(w), 48, 0, None), _abi.ERR_INVALID, b"null net_out")
    w18 = _weights(17, self_dim=18)
    _refused(L.ebc_sarl_net_create_om(C.addressof(w18), 48, 0, C.byref(out)), _abi.ERR_UNSUPPORTED, b"self_state_dim 18")
    # a spec that passes every check reaches the weights: NULL ones are named
    _refused(L.ebc_sarl_net_create_om(C.addressof(w), 48, 0, C.byref(out)), _abi.ERR_INVALID, b"null weight or bias of layer 1")
    assert not out.value


def test_handle_entries_refuse_null_arguments_without_a_device():
    L = _capi.lib()
    spec = _abi.om_spec(OccupancySpec(4, 1.0, 3))
    buf = np.zeros(8)
    _refused(L.ebc_observe_wide(None, C.addressof(spec), buf.ctypes.data, None), _abi.ERR_INVALID, b"null handle")
    args = _abi.EbcStepKArgs()
    args.struct_size = C.sizeof(args)
    om = _abi.EbcStepKOm()
    om.struct_size, om.spec, om.state_wide = C.sizeof(om), spec, buf.ctypes.data
    _refused(L.ebc_step_k_om(None, C.addressof(args), C.addressof(om)), _abi.ERR_INVALID, b"null handle")
    _refused(L.ebc_step_k_om(None, C.addressof(args), None), _abi.ERR_INVALID, b"ebc_step_k_om: om is NULL")
    _refused(L.ebc_observe_wide(None, None, buf.ctypes.data, None), _abi.ERR_INVALID, b"EbcOmSpec.struct_size")
    # a bad struct_size of either new struct is named before the handle is looked at
    short = _abi.om_spec(OccupancySpec(4, 1.0, 3))
    short.struct_size -= 8
    _refused(L.ebc_observe_wide(None, C.addressof(short), buf.ctypes.data, None), _abi.ERR_INVALID, b"EbcOmSpec.struct_size")
    om.struct_size += 8
    _refused(L.ebc_step_k_om(None, C.addressof(args), C.addressof(om)), _abi.ERR_INVALID, b"EbcStepKOm.struct_size")
    om.struct_size, om.spec = C.sizeof(om), short
    _refused(L.ebc_step_k_om(None, C.addressof(args), C.addressof(om)), _abi.ERR_INVALID, b"EbcOmSpec.struct_size")


def test_trainer_and_schedule_refuse_a_width_that_does_not_match():
    from ebcsim.sarl_train import run_sarl_training
    wnet = oc.NARROW_WIDE[1]
    sd = sg.random_state_dict(wnet[0])
    with pytest.raises(NotImplementedError, match="om_width 193"):
        SarlTrainer(sd, device="cpu", native=False, om_width=193)
    with pytest.raises(NotImplementedError, match="om_width -1"):
        SarlTrainer(sd, device="cpu", native=False, om_width=-1)
    with pytest.raises(NotImplementedError, match="T \\+ om_width = 225"):
        SarlTrainer(sg.random_state_dict(oc.wide_net(33, 192)[0]), device="cpu", native=False, om_width=192)
    with pytest.raises(NotImplementedError, match="needs a HIP device"):
        SarlTrainer(sd, device="cpu", native=True, om_width=48)

    class Env(object):
        T, R, E = 17, 5, 4

    class OnDevice(object):  # the schedule looks at the device's type before anything else
        def __init__(self, tr):
            self.__dict__.update(tr.__dict__)
            self.device = torch.device("cuda", 0)
            self.native = False
    tr = OnDevice(SarlTrainer(sd, device="cpu", native=False, om_width=48))
    with pytest.raises(NotImplementedError, match="rows are 17 wide and the occupancy maps 27, the network takes 65 \\(48 of them maps\\)"):
        run_sarl_training(Env(), tr, np.zeros((3, 2)), 0.9, om=OccupancySpec(3, 1.0, 3))
    with pytest.raises(NotImplementedError, match="rows are 17 wide and the occupancy maps 0, the network takes 65"):
        run_sarl_training(Env(), tr, np.zeros((3, 2)), 0.9)
    plain = OnDevice(SarlTrainer(sg.random_state_dict(sg.NARROW_T17_NET), device="cpu", native=False))
    with pytest.raises(NotImplementedError, match="the occupancy maps 48, the network takes 17"):
        run_sarl_training(Env(), plain, np.zeros((3, 2)), 0.9, om=OccupancySpec(4, 1.0, 3))


# ---------------------------------------------------------------------- the C ABI
NEW_ENTRIES = (("ebc_observe_wide", 4), ("ebc_step_k_om", 3), ("ebc_sarl_net_create_om", 4))


def test_bindings_match_the_header():
    text = open(HEADER).read()
    for name, n_args in NEW_ENTRIES:
        m = re.search(r"^int %s\(([^)]*)\);" % name, text, flags=re.M)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int and hasattr(_capi.lib(), name)


@pytest.mark.parametrize("name", ["EbcOmSpec", "EbcStepKOm"])
def test_struct_layouts_match_the_header(name, tmp_path):
    S = getattr(_abi, name)
    fields = [f for f, _ in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",sizeof(%s));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, name, "\n".join('printf(" %%zu",offsetof(%s,%s));' % (name, f) for f in fields)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", exe], check=True, timeout=120)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert sizes == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


def test_project_config_asks_for_the_reference_maps():
    import configparser
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_om.config"))
    spec = OccupancySpec.from_config(cfg)
    assert spec == OccupancySpec(4, 1.0, 3) and spec.width == 48 and cfg.getboolean("sarl", "with_om")
