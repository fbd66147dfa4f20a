"""Training LSTM-RL without a GPU: the packed layout and its round trip into LstmModule, the host build of the gradient rule
(csrc/ebc_lstm_grad_rule.h) against float64 autograd of LstmModule per parameter tensor, b_ih and b_hh, the edge batches,
the host program under the sanitizers, sort_rows_by_distance against the reference's order, and the autograd trainer
against plain torch.  Cases and the bar: tests/lstm_grad_cases.py."""
import subprocess

import numpy as np
import pytest
import torch

from lstm_grad_cases import (BATCHES, NARROW_NET1, NARROW_NET2, NETS, REFERENCE_NET1, REFERENCE_NET2, ROWS, TOL_FACTOR, YARDSTICK_FLOOR,
                             accuracy_cases, accuracy_row, batches, case_name, chunk, edge_batch, golden_rows, host_floats, host_grad, host_layers,
                             host_lib, host_pack, host_program, is_live, module, plain_batch, random_state_dict, read_results, same_bytes,
                             torch_grad, unpacked, write_batches, _w)
from lstm_cases import RUNS


def test_the_packed_layout_is_the_headers():
    from ebcsim.lstm_train import packed_floats
    assert chunk() == 4 and batches() == BATCHES
    assert host_floats(REFERENCE_NET2) == packed_floats(*REFERENCE_NET2) == 87248
    assert host_floats(REFERENCE_NET1) == packed_floats(*REFERENCE_NET1) == 47268
    for net in NETS:
        assert host_floats(net) == packed_floats(*net)
    lay = host_layers(REFERENCE_NET2)
    assert [op for _, _, op in lay] == [152, 100, 100, 52, 152, 100, 100, 4, 200]
    assert [k for _, k, _ in lay] == [13, 150, 100, 100, 56, 150, 100, 100, 101]
    assert [at for at, _, _ in host_layers(REFERENCE_NET1)][:4] == [0, 0, 0, 0] and host_layers(REFERENCE_NET1)[8][0] == 0


@pytest.mark.parametrize("ni", range(4))
def test_pack_round_trip_loads_strict(ni, tmp_path):
    """pack_state_dict gives the header's image byte for byte (pad entries 0); unpack_to_state_dict gives the tensors back,
    and the file LstmTrainer.save writes loads into LstmModule with strict=True."""
    from ebcsim.lstm_rl import LstmModule
    from ebcsim.lstm_train import LstmTrainer, module_of, pack_state_dict, shape_of, unpack_to_state_dict
    net = NETS[ni]
    sd = random_state_dict(net, scale=1.0)
    assert shape_of(sd) == net
    flat = pack_state_dict(sd)
    assert same_bytes(flat.numpy(), host_pack(sd))
    back = unpack_to_state_dict(flat, *net)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) and back[k].is_contiguous() for k in sd)
    assert int((flat != 0).sum()) == sum(int((v != 0).sum()) for v in sd.values())  # nothing but the tensors: the pads are 0
    module(net).load_state_dict(back, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in module_of(back).state_dict().items())
    tr = LstmTrainer(sd, device="cpu")
    assert tr.native is False and tr.net is None and tr.widths == net[0] and tr.with_interaction_module == net[2]
    path = str(tmp_path / "model.pth")
    tr.save(path)
    loaded = torch.load(path, map_location="cpu")
    LstmModule.from_state_dict(loaded, net[1])  # strict inside
    assert all(torch.equal(loaded[k], sd[k]) for k in sd)


@pytest.mark.parametrize("case", accuracy_cases(), ids=case_name)
def test_the_rule_against_float64_autograd(case):
    """Per parameter tensor and for the loss the host build's error against float64 autograd of LstmModule is within
    TOL_FACTOR times torch's own float32 error against the same float64 run.  A yardstick below 2^-25 is none: no float32
    result can be held under half a unit of its last place, and torch's landing closer than that is luck (the seeded cases
    draw another seed then; a golden run has one batch, so there the floor stands in: lstm_interaction_n10's mlp.6.bias,
    ONE number, torch 2.0e-9, the rule 8.9e-8 = one and a half units, profiles/lstm_grad_accuracy.txt)."""
    tensors, (lr, lt), seed = accuracy_row(case)
    for key, er, et in tensors + [("loss_sum", lr, lt)]:
        print("%-22s rule %.3e torch32 %.3e ratio %.2f" % (key, er, et, er / et if et else float("inf")))
    for key, er, et in tensors + [("loss_sum", lr, lt)]:
        assert et >= YARDSTICK_FLOOR or case[0] == "golden", (key, et)
        assert er <= TOL_FACTOR * max(et, YARDSTICK_FLOOR), (case, key, er, et)


@pytest.mark.parametrize("ni", [2, 3, 0])
def test_b_ih_and_b_hh_receive_the_same_bytes(ni):
    net = NETS[ni]
    sd = random_state_dict(net, scale=4.0)
    rows, target = plain_batch(net, 9, 5)
    g, loss, count, value, joint = host_grad(host_pack(sd), net, rows, target, grad_scale=2.0 / 9)
    at, k, h4 = host_layers(net)[8]
    b_ih, b_hh = g[at + (k - 1) * h4:at + k * h4], g[at + k * h4:at + (k + 1) * h4]
    assert same_bytes(b_ih, b_hh) and np.abs(b_ih).max() > 0 and count == 9
    got = unpacked(net, g)
    assert same_bytes(got["lstm.bias_ih_l0"], got["lstm.bias_hh_l0"])


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("ni", [2, 3])
def test_edge_batches(ni, R):
    """n_valid of 0, 1, R, R + 3 and -1, masks, NaN in every padding row and in masked states: what is not live enters no
    sum, padding rows are never read (the bytes are those of the same batch with the padding zeroed), the values of states
    without rows are NaN and their joint vectors 0, and the gradient agrees with float64 autograd over the live states."""
    net = NETS[ni]
    sd = random_state_dict(net)
    P = host_pack(sd)
    for B in BATCHES:
        rows, target, nv, mask, kinds = edge_batch(net, B, R)
        got = host_grad(P, net, rows, target, nv, mask, 2.0 / B)
        live = is_live(nv, mask)
        assert got[2] == int(live.sum()), kinds
        n = np.clip(nv, 0, R)
        assert np.isnan(got[3][n == 0]).all() and (got[4][n == 0].view(np.uint32) == 0).all()
        clean = rows.copy()
        clean[np.arange(R)[None, :] >= n[:, None]] = 0.0
        again = host_grad(P, net, clean, target, n, mask, 2.0 / B)
        assert all(same_bytes(a, b) for a, b in zip((got[0], got[3], got[4]), (again[0], again[3], again[4]))) and got[1] == again[1]
        if not live.any():
            assert got[1] == 0.0 and (got[0].view(np.uint32) == 0).all()
            continue
        assert np.isfinite(got[0]).all() and np.isfinite(got[1])
        g64, l64, v64 = torch_grad(sd, rows, target, nv, live, 2.0 / B, torch.float64)
        mine = unpacked(net, got[0])
        for k in g64:
            np.testing.assert_allclose(mine[k], g64[k], rtol=0, atol=2e-5 * max(np.abs(g64[k]).max(), 1e-30), err_msg="%s %s" % (k, kinds))
        np.testing.assert_allclose(got[3][live], v64, rtol=0, atol=1e-5)
        assert abs(got[1] - l64) <= 1e-5 * max(l64, 1e-30)


def test_a_nan_in_a_live_row_reaches_loss_and_grad_and_nothing_of_a_dead_one_does():
    net = NARROW_NET2
    sd = random_state_dict(net)
    P = host_pack(sd)
    rows, target = plain_batch(net, 7, 2, seed=91)
    clean = host_grad(P, net, rows, target, None, None, 0.1)
    rows[5, 1, 3] = np.nan
    got = host_grad(P, net, rows, target, None, None, 0.1)
    assert np.isnan(got[1]) and np.isnan(got[0]).any() and got[2] == 7
    assert (got[0][np.isnan(got[0])].view(np.uint32) == 0x7FC00000).all() and got[3].view(np.uint32)[5] == 0x7FC00000
    mask = np.ones(7, dtype=np.uint8)
    mask[5] = 0
    dead = host_grad(P, net, rows, target, None, mask, 0.1)
    assert dead[2] == 6 and np.isfinite(dead[0]).all() and np.isfinite(dead[1]) and dead[1] < clean[1]
    none = host_grad(P, net, rows, target, None, np.zeros(7, dtype=np.uint8), 0.1)
    assert none[2] == 0 and none[1] == 0.0 and (none[0].view(np.uint32) == 0).all()


def test_the_limits_of_the_header():
    L = host_lib()
    ref2, ref1 = REFERENCE_NET2[0], REFERENCE_NET1[0]

    def code(widths, S=6, two=1, **kw):
        w = list(widths)
        for i, v in kw.items():
            w[int(i[1:])] = v
        return int(L.lstm_grad_host_refused(_w(w).ctypes.data, S, two))
    assert code(ref2) == 0 and code(ref1, two=0) == 0
    assert code(ref2, w0=65) == 1 and code(ref2, w0=0) == 1 and code(ref2, w0=64) == 0
    assert code(ref2, w1=257) == 2 and code(ref2, w3=0) == 4 and code(ref2, w2=256) == 0
    assert code(ref2, w4=65) == 6 and code(ref2, w4=64) == 0
    assert code(ref2, w5=65) == 7 and code(ref2, w5=0) == 7 and code(ref2, w5=64) == 0
    assert code(ref2, w6=257) == 8 and code(ref2, w8=0) == 10 and code(ref2, w9=2) == 11 and code(ref2, w7=256) == 0
    assert code(ref2, S=14) == 12 and code(ref2, S=-1) == 12 and code(ref2, S=13) == 0 and code(ref2, S=0) == 0
    assert code(ref1, two=0, w0=64) == 0 and code(ref1, two=0, w1=9999) == 0  # mlp1's widths are not read without mlp1


def test_host_program_under_the_sanitizers(tmp_path):
    """The rule as a program of its own, built with -fsanitize=address,undefined, on plain and edge batches of both narrow
    networks and one reference-width batch: it ends clean and writes the library build's bytes."""
    batch_list, want = [], []
    for net, shapes in ((NARROW_NET2, [(B, R) for B in BATCHES for R in ROWS]), (NARROW_NET1, [(9, 5), (3, 1)]), (REFERENCE_NET2, [(5, 2)]),
                        (REFERENCE_NET1, [(1, 10)])):
        P = host_pack(random_state_dict(net))
        for B, R in shapes:
            rows, target, nv, mask, _ = edge_batch(net, B, R)
            batch_list.append((net, P, rows, target, nv, mask, 2.0 / B))
            want.append(host_grad(P, net, rows, target, nv, mask, 2.0 / B))
            rows, target = plain_batch(net, B, R)
            batch_list.append((net, P, rows, target, None, None, 2.0 / B))
            want.append(host_grad(P, net, rows, target, None, None, 2.0 / B))
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_batches(src, batch_list)
    run = subprocess.run([host_program(sanitize=True), src, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert run.returncode == 0, run.stdout.decode()
    for got, w in zip(read_results(out, batch_list), want):
        assert same_bytes(got[0], w[0]) and np.float64(got[1]).tobytes() == np.float64(w[1]).tobytes() and got[2] == w[2]
        assert same_bytes(got[3], w[3]) and same_bytes(got[4], w[4])


# ---------------------------------------------------------------------------------------------- sort_rows_by_distance
@pytest.mark.parametrize("name", RUNS)
def test_sort_gives_the_recorded_order_on_the_golden_states(name):
    """The golden runs' last_state is what LstmRL.sorted_order made of the env's rows.  Shuffled (seeded) and sorted again on
    the float32 distance column they are the recorded rows, byte for byte, wherever no two distances of a state are equal
    in float32 (no state of the golden runs has such a pair: asserted)."""
    from ebcsim.lstm_train import DISTANCE_COLUMN, sort_rows_by_distance
    _, rows, _ = golden_rows(name)
    N, R, _ = rows.shape
    da = rows[:, :, DISTANCE_COLUMN]
    assert (np.diff(da, axis=1) < 0).all()  # recorded in strictly decreasing float32 distance
    rs = np.random.RandomState(5)
    shuffled = np.stack([rows[i][rs.permutation(R)] for i in range(N)])
    assert not same_bytes(shuffled, rows)
    got = sort_rows_by_distance(torch.from_numpy(shuffled))
    assert same_bytes(got.numpy(), rows)
    nv = torch.from_numpy(rs.randint(0, R + 1, N).astype(np.int64))
    got = sort_rows_by_distance(torch.from_numpy(shuffled), nv).numpy()
    for i in range(N):
        n = int(nv[i])
        assert same_bytes(got[i, n:], shuffled[i, n:])  # a padding row stays where it is
        want = shuffled[i, :n][np.argsort(-shuffled[i, :n, DISTANCE_COLUMN], kind="stable")]
        assert same_bytes(got[i, :n], want)


def test_sort_is_the_policys_order_and_keeps_a_tie():
    """LstmRL.sorted_order on a constructed state with two agents mirrored about the robot (the same distance exactly) and
    a third at that distance: sort_rows_by_distance of the env-ordered rows is the rows in the policy's order, the tied rows
    in their original order."""
    from ebcsim.agents import AgentType
    from ebcsim.lstm_train import DISTANCE_COLUMN, sort_rows_by_distance
    from ebcsim.rl_policy import LstmRL
    from ebcsim.state import FullState, JointState, ObservableState
    me = FullState(0.0, 0.0, 0.0, 0.0, 0.3, 0.0, 4.0, 1.0, 0.0)
    others = [ObservableState(px, py, 0, 0, 0.3, AgentType.ADULT) for px, py in ((3.0, 4.0), (1.0, 0.0), (-3.0, -4.0), (0.0, 6.0), (5.0, 0.0))]
    st = JointState(me, list(others))
    order = LstmRL.sorted_order(st)
    assert order == [3, 0, 2, 4, 1]
    pol = LstmRL()
    pol.kinematics, pol.device = "holonomic", torch.device("cpu")
    rows_env = pol.transform(st)
    assert float(rows_env[0, DISTANCE_COLUMN]) == float(rows_env[2, DISTANCE_COLUMN]) == float(rows_env[4, DISTANCE_COLUMN]) == 5.0
    got = sort_rows_by_distance(rows_env[None])
    assert same_bytes(got[0].numpy(), rows_env[order].numpy())


def test_sort_never_moves_a_padding_row_forward():
    from ebcsim.lstm_train import DISTANCE_COLUMN, sort_rows_by_distance
    rs = np.random.RandomState(3)
    rows = rs.normal(0, 1, (6, 5, 13)).astype(np.float32)
    rows[:, :, DISTANCE_COLUMN] = np.abs(rows[:, :, DISTANCE_COLUMN])
    nv = np.array([0, 1, 3, 5, 2, 4], dtype=np.int64)
    for b in range(6):  # padding that would win every comparison, and padding that compares with nothing
        rows[b, nv[b]:, DISTANCE_COLUMN] = (1e30, np.inf, np.nan)[b % 3]
    rows[3, 1, DISTANCE_COLUMN] = np.nan  # an existing row without a distance goes behind the existing ones, before the padding
    got = sort_rows_by_distance(torch.from_numpy(rows), torch.from_numpy(nv)).numpy()
    for b in range(6):
        n = int(nv[b])
        assert same_bytes(got[b, n:], rows[b, n:])
        assert sorted(map(bytes, got[b, :n])) == sorted(map(bytes, rows[b, :n]))
        d = got[b, :n, DISTANCE_COLUMN]
        d = d[~np.isnan(d)]
        assert (np.diff(d) <= 0).all()
    assert np.isnan(got[3, 4, DISTANCE_COLUMN])


# ---------------------------------------------------------------------------------------------- the autograd trainer
@pytest.mark.parametrize("ni", [2, 3])
def test_autograd_trainer_takes_three_sgd_steps_like_plain_torch(ni):
    """LstmTrainer(native=False): three SGD steps (momentum 0.9) on an edge batch move the weights exactly as
    torch.optim.SGD moves LstmModule's parameters on the same loss."""
    from ebcsim.lstm_train import LstmTrainer, module_of
    net = NETS[ni]
    sd = random_state_dict(net)
    rows, target, nv, mask, _ = edge_batch(net, 9, 5)
    target = np.nan_to_num(target)
    live = is_live(nv, mask)
    tr = LstmTrainer(sd, device="cpu", optimizer="sgd", lr=0.05, native=False)
    assert tr.flat.is_leaf and tr.flat.requires_grad
    m = module_of(sd)
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
    idx = np.nonzero(live)[0]
    x = torch.from_numpy(rows[idx].copy())
    n = torch.from_numpy(np.clip(nv[idx], 0, 5))
    x[torch.arange(5)[None, :] >= n[:, None]] = 0.0
    y = torch.from_numpy(target[idx])
    for step in range(3):
        loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
        tr.step()
        opt.zero_grad()
        d = m(x, n).squeeze(1) - y
        (0.5 * (2.0 / len(idx)) * (d * d).sum()).backward()
        opt.step()
        assert int(count) == len(idx) and abs(float(loss) - float((d.detach().double() ** 2).sum())) <= 1e-12
        now = tr.state_dict()
        for k, v in m.state_dict().items():
            assert torch.equal(now[k], v), (step, k)
    assert not all(torch.equal(now[k], sd[k]) for k in sd)
    with pytest.raises(NotImplementedError):
        LstmTrainer(sd, device="cpu", native=True)
    with pytest.raises(ValueError):
        tr.loss_and_grad(torch.zeros(1, 2, 14), torch.zeros(1))


def test_refresh_from_on_the_cpu_copies_the_weights():
    from ebcsim.lstm_rl import LstmValueNet
    from ebcsim.lstm_train import LstmTrainer
    net = NARROW_NET2
    sd = random_state_dict(net)
    tr = LstmTrainer(sd, device="cpu", lr=0.05)
    vn = LstmValueNet(sd, device="cpu")
    rows, target = plain_batch(net, 5, 3)
    v0 = vn.forward(torch.from_numpy(rows)).clone()
    tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target))
    tr.step()
    assert vn.refresh_from(tr) is False and vn.native_refreshes == 0  # no blocks on the CPU
    fresh = LstmValueNet(tr.state_dict(), device="cpu")
    v1 = vn.forward(torch.from_numpy(rows))
    assert torch.equal(v1, fresh.forward(torch.from_numpy(rows))) and not torch.equal(v1, v0)
