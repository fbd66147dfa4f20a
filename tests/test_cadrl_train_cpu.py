"""Training CADRL without a GPU: the host build of the gradient rule (csrc/ebc_cadrl_grad_rule.h) against torch's autograd
of CadrlModule, its edges stated one by one (a tie of the minimum, rows past n_valid, row counts of 0, below 0 and above R,
masked states, a batch without a live state, a NaN in a live row), the chunk sums against a plain restatement, the host
program under the sanitizers, the reference's own Trainer steps (tests/golden/cadrl_one_trainer_steps.npz) and the C ABI's
declarations.  Cases and the bar: tests/cadrl_grad_cases.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cadrl_cases import TOL_FACTOR
from cadrl_grad_cases import (BATCHES, NARROW_WIDTHS, REFERENCE_WIDTHS, WIDTHS, accuracy_cases, accuracy_row, chunk, edge_batch,
                              host_floats, host_grad, host_layers, host_pack, host_program, is_live, layer_slices, plain_batch,
                              random_state_dict, read_results, row_values, same_bytes, torch_grad, write_batches)
from helpers import load
from ebcsim import _abi, _capi
from ebcsim.cadrl import CadrlModule, CadrlValueNet
from ebcsim.cadrl_train import (LAYER_KEYS, CadrlTrainer, pack_state_dict, packed_floats, unpack_to_state_dict, widths_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")
NAN32, NAN64 = 0x7fc00000, 0x7ff8000000000000


@pytest.mark.parametrize("wi,B,R", accuracy_cases())
def test_host_build_against_float64_autograd(wi, B, R):
    """Per layer and for the loss: the rule's error against float64 autograd is within TOL_FACTOR times the error of
    torch's own float32 autograd on the same weights and inputs.  Precondition, for every state: the float64 top-2 gap of
    its rows exceeds twice the tolerance of the values, and the rule took the row float64 takes."""
    layers, (loss_rule, loss_t32), (gap, tol), (picked, picked64), seed = accuracy_row(wi, B, R)
    for name, err_rule, err_t32 in layers + [("loss_sum", loss_rule, loss_t32)]:
        print("widths %s B %3d R %d seed %d %-16s rule %.3e torch32 %.3e" % (WIDTHS[wi], B, R, seed, name, err_rule, err_t32))
    assert gap > 2 * tol, (gap, tol)
    assert (picked == picked64).all()
    for name, err_rule, err_t32 in layers:
        assert err_rule <= TOL_FACTOR * err_t32, (name, err_rule, err_t32)
    assert loss_rule <= TOL_FACTOR * loss_t32, (loss_rule, loss_t32)


def test_packed_layout_is_the_documented_one():
    """W[k][units padded to a multiple of 4] then the bias, layer after layer; 27 732 floats at the reference widths; the
    python packer, the header's packer and unpack agree; pad entries are exactly 0."""
    assert host_floats(REFERENCE_WIDTHS) == packed_floats(REFERENCE_WIDTHS) == 27732
    assert [op for _, op in host_layers(REFERENCE_WIDTHS)] == [152, 100, 100, 4]
    for widths in WIDTHS:
        sd = random_state_dict(widths)
        assert widths_of(sd) == widths
        flat = pack_state_dict(sd)
        assert same_bytes(flat.numpy(), host_pack(sd)) and flat.numel() == host_floats(widths)
        at = 0
        for (k, o), key, (off, op) in zip(zip(widths[:-1], widths[1:]), LAYER_KEYS, host_layers(widths)):
            assert off == at and op == (o + 3) // 4 * 4
            W = flat[at:at + k * op].view(k, op)
            assert torch.equal(W[:, :o], sd[key + ".weight"].t()) and bool((W[:, o:] == 0).all())
            assert torch.equal(flat[at + k * op:at + k * op + o], sd[key + ".bias"]) and bool((flat[at + k * op + o:at + (k + 1) * op] == 0).all())
            at += (k + 1) * op
        back = unpack_to_state_dict(flat, widths)
        assert list(back) == list(CadrlModule(widths[0], widths[1:]).state_dict()) and all(torch.equal(back[k], sd[k]) for k in sd)


# ---------------------------------------------------------------------- edge states, one by one
def _net(widths=NARROW_WIDTHS):
    sd = random_state_dict(widths)
    return widths, sd, host_pack(sd)


def test_a_tie_of_the_minimum_goes_to_the_first_row():
    widths, sd, P = _net()
    rows, target = plain_batch(widths, 6, 5, seed=61)
    v = row_values(sd, rows, torch.float32)
    pairs = []
    for b in range(6):  # the minimal row's bytes copied to another row, before it or behind it; in state 0 the pair ends at row 4
        r = int(np.argmin(v[b]))
        other = ((0 if r == 4 else 4) if b == 0 else (r + 1 + b % 4) % 5)
        rows[b, other] = rows[b, r]
        pairs.append((min(r, other), max(r, other)))
    assert any(p[0] != int(np.argmin(v[b])) for b, p in enumerate(pairs)) and any(p[0] == int(np.argmin(v[b])) for b, p in enumerate(pairs))
    g, loss, count, value, min_row = host_grad(P, widths, rows, target, grad_scale=1.0)
    assert count == 6 and [int(r) for r in min_row] == [p[0] for p in pairs]
    # every output is the one of the batch whose later tied row holds the state's LARGEST row instead: nothing of it enters
    rows2 = rows.copy()
    for b, (first, later) in enumerate(pairs):
        top = int(np.argmax(np.where((np.arange(5) == later) | (np.arange(5) == first), -np.inf, v[b])))
        assert top not in (first, later) and v[b, top] > v[b].min()
        rows2[b, later] = rows[b, top]
    g2, loss2, _, value2, min_row2 = host_grad(P, widths, rows2, target, grad_scale=1.0)
    assert same_bytes(min_row, min_row2) and same_bytes(g, g2) and loss == loss2 and same_bytes(value, value2)
    # and of the batch with the later tied row cut off, where it is the last row (state 0 by construction)
    cut = 0
    for b, (first, later) in enumerate(pairs):
        if later == 4:
            nv = np.full(6, 5, dtype=np.int64)
            nv[b] = 4
            g3, loss3, _, value3, min_row3 = host_grad(P, widths, rows, target, nv, grad_scale=1.0)
            assert same_bytes(g, g3) and loss == loss3 and same_bytes(value, value3) and same_bytes(min_row, min_row3)
            cut += 1
    assert cut >= 1 and pairs[0][1] == 4


def test_rows_past_n_valid_reach_nothing():
    """NaN and both infinities in the rows at or past n_valid: every output has the bytes of the same batch with zeros
    there, and of the batch cut to the valid rows where every state has the same count."""
    widths, sd, P = _net()
    B, R = chunk() + 3, 5
    rows, target = plain_batch(widths, B, R, seed=62)
    nv = np.array([1 + b % (R - 1) for b in range(B)], dtype=np.int64)
    clean = rows.copy()
    for b in range(B):
        for r in range(int(nv[b]), R):
            rows[b, r] = (np.nan, np.inf, -np.inf)[(r + b) % 3]
            clean[b, r] = 0.0
    bad, good = host_grad(P, widths, rows, target, nv, grad_scale=2.0 / B), host_grad(P, widths, clean, target, nv, grad_scale=2.0 / B)
    assert np.isfinite(bad[0]).all() and np.abs(bad[0]).max() > 0 and np.isfinite(bad[1]) and bad[2] == B
    assert same_bytes(bad[0], good[0]) and bad[1] == good[1] and same_bytes(bad[3], good[3]) and same_bytes(bad[4], good[4])
    assert (bad[4] < nv).all() and (bad[4] >= 0).all()
    two = np.full(B, 2, dtype=np.int64)
    rows = clean.copy()
    rows[:, 2:] = np.nan
    cut = host_grad(P, widths, np.ascontiguousarray(rows[:, :2]), target, None, grad_scale=2.0 / B)
    full = host_grad(P, widths, rows, target, two, grad_scale=2.0 / B)
    assert np.isfinite(cut[0]).all() and same_bytes(cut[0], full[0]) and cut[1] == full[1] and same_bytes(cut[3], full[3]) and same_bytes(cut[4], full[4])


def test_n_valid_of_zero_negative_and_above_r():
    widths, sd, P = _net()
    rows, target = plain_batch(widths, 4, 3, seed=63)
    nv = np.array([0, -5, 3 + 7, 3], dtype=np.int64)
    poisoned = rows.copy()
    poisoned[:2] = np.nan  # a state without rows reads none of them
    g, loss, count, value, min_row = host_grad(P, widths, poisoned, target, nv, grad_scale=1.0)
    assert count == 2 and np.isfinite(g).all() and np.isfinite(loss)
    assert (value[:2].view(np.uint32) == NAN32).all() and (min_row[:2] == -1).all()
    # above R counts as R: states 2 and 3 alone, with all their rows
    g2, loss2, count2, value2, min_row2 = host_grad(P, widths, rows[2:], target[2:], None, grad_scale=1.0)
    assert same_bytes(g, g2) and loss == loss2 and count2 == 2 and same_bytes(value[2:], value2) and same_bytes(min_row[2:], min_row2)


def test_sample_mask_zero_enters_no_sum():
    widths, sd, P = _net()
    B = chunk() + 5
    rows, target = plain_batch(widths, B, 2, seed=64)
    mask = np.array([b % 3 != 1 for b in range(B)], dtype=np.uint8)
    poisoned, ptarget = rows.copy(), target.copy()
    poisoned[mask == 0, 1, 4] = np.nan
    poisoned[mask == 0, 0, 0] = np.inf
    ptarget[mask == 0] = np.nan
    a, b = host_grad(P, widths, poisoned, ptarget, None, mask, grad_scale=0.25), host_grad(P, widths, rows, target, None, mask, grad_scale=0.25)
    assert np.isfinite(a[0]).all() and same_bytes(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] == int(mask.sum())
    assert same_bytes(a[3][mask != 0], b[3][mask != 0]) and (a[3][mask == 0].view(np.uint32) == NAN32).all()
    # against float64 autograd of the live states alone
    g64, l64, _ = torch_grad(sd, rows, target, None, mask != 0, 0.25, torch.float64)
    np.testing.assert_allclose(a[0], g64, rtol=0, atol=2e-5 * np.abs(g64).max())
    assert abs(a[1] - l64) <= 1e-5 * l64


def test_a_batch_with_no_live_state():
    widths, sd, P = _net()
    B = chunk() + 2
    rows, target = plain_batch(widths, B, 3, seed=65)
    for kw in (dict(mask=np.zeros(B, np.uint8)), dict(n_valid=np.zeros(B, np.int64)), dict(n_valid=np.full(B, -1, np.int64))):
        g, loss, count, value, min_row = host_grad(P, widths, rows, target, grad_scale=0.5, **kw)
        assert count == 0 and loss == 0.0 and (g.view(np.uint32) == 0).all()
    g, loss, count, _, _ = host_grad(P, widths, rows[:0], target[:0])
    assert count == 0 and loss == 0.0 and (g.view(np.uint32) == 0).all()


def test_a_nan_in_a_live_row_reaches_the_loss_and_the_gradient():
    widths, sd, P = _net()
    rows, target = plain_batch(widths, 5, 2, seed=66)
    rows[3, 1, 7] = np.nan
    g, loss, count, value, min_row = host_grad(P, widths, rows, target, grad_scale=0.4)
    assert count == 5 and np.isnan(loss) and np.float64(loss).view(np.uint64) == NAN64
    assert value[3:4].view(np.uint32)[0] == NAN32 and min_row[3] == 1 and np.isfinite(np.delete(value, 3)).all()
    assert np.isnan(g).any() and (g[np.isnan(g)].view(np.uint32) == NAN32).all()
    s = layer_slices(widths)[3]
    assert np.isnan(g[s][:widths[3] * 4:4]).all()  # the last layer's weights: the seed times the kept activations


# ---------------------------------------------------------------------- chunking
_LD = np.longdouble  # 64 bits of mantissa: a float32 product is exact in it and a + of a float32 rounds far below float32's half spacing


def _fma32(a, b, c):
    """fmaf on float32 arrays: the exact product plus c, rounded to float32 once."""
    return (np.asarray(a, dtype=np.float32).astype(_LD) * np.asarray(b, dtype=np.float32).astype(_LD)
            + np.asarray(c, dtype=np.float32).astype(_LD)).astype(np.float32)


def _restated(sd, widths, rows, target, nv, mask, scale):
    """The rule in plain numpy, written from its text: a unit's chain over its inputs ascending from 0 and then + bias,
    ReLU, the minimum over a state's rows and its first row, d = value - target, the seed scale * d, the Linear and ReLU
    backward, every weight's chain over a chunk's live states ascending from 0, the chunks of 16 added in float64 and
    rounded once; the loss in float64.  -> (grad in the packed layout, loss_sum, count, and of the live states value [B], min_row [B])."""
    f32 = np.float32
    W = [sd[k + ".weight"].numpy().T.astype(f32) for k in LAYER_KEYS]  # [K][O]
    bias = [sd[k + ".bias"].numpy().astype(f32) for k in LAYER_KEYS]

    def forward(x):
        acts = [x.astype(f32)]
        for l in range(4):
            acc = np.zeros(widths[l + 1], dtype=f32)
            for k in range(widths[l]):
                acc = _fma32(acts[-1][k], W[l][k], acc)
            y = acc + bias[l]
            acts.append(np.where(y < 0, f32(0), y) if l < 3 else y)
        return acts

    B, R, _ = rows.shape
    total = [(np.zeros(w.shape, np.float64), np.zeros(b.shape, np.float64)) for w, b in zip(W, bias)]
    loss, count, value, min_row = 0.0, 0, np.full(B, np.nan, dtype=f32), np.full(B, -1, dtype=np.int32)
    for c0 in range(0, B, 16):
        G = [(np.zeros(w.shape, f32), np.zeros(b.shape, f32)) for w, b in zip(W, bias)]
        chunk_loss = 0.0
        for b in range(c0, min(B, c0 + 16)):
            n = R if nv is None else max(0, min(R, int(nv[b])))
            if n < 1 or (mask is not None and not mask[b]):
                continue  # not live: nothing of it is looked at
            v = np.array([forward(rows[b, r])[4][0] for r in range(n)], dtype=f32)
            assert np.isfinite(v).all()
            r = int(np.argmin(v))  # numpy's first minimum
            value[b], min_row[b] = v[r], r
            acts = forward(rows[b, r])
            d = f32(v[r] - f32(target[b]))
            chunk_loss, count = chunk_loss + float(d) * float(d), count + 1
            delta = np.array([f32(scale) * d], dtype=f32)
            for l in (3, 2, 1, 0):
                x = acts[l]
                G[l] = (_fma32(delta[None, :], x[:, None], G[l][0]), G[l][1] + delta)
                if l:
                    dx = np.zeros(widths[l], dtype=f32)
                    for u in range(widths[l + 1]):
                        dx = _fma32(W[l][:, u], delta[u], dx)
                    delta = np.where(x > 0, dx, f32(0))
        total = [(tw + gw.astype(np.float64), tb + gb.astype(np.float64)) for (tw, tb), (gw, gb) in zip(total, G)]
        loss = loss + chunk_loss
    flat, at = np.zeros(packed_floats(widths), dtype=f32), 0
    for l, (tw, tb) in enumerate(total):
        K, O = widths[l], widths[l + 1]
        Op = (O + 3) // 4 * 4
        flat[at:at + K * Op].reshape(K, Op)[:, :O] = tw.astype(f32)
        flat[at + K * Op:at + K * Op + O] = tb.astype(f32)
        at += (K + 1) * Op
    return flat, loss, count, value, min_row


@pytest.mark.parametrize("B", BATCHES)
def test_chunk_sums_against_a_plain_restatement(B):
    """B = 1, 15, 16, 17, 33: the host build gives the bytes of the rule restated in numpy (chains and chunk sums written
    out in the test), on an edge batch: gradient, loss, count, values and rows."""
    assert chunk() == 16
    widths, sd, P = _net()
    rows, target, nv, mask, kinds = edge_batch(widths, B, 3, seed=70 + B)
    got = host_grad(P, widths, rows, target, nv, mask, grad_scale=0.125)
    want = _restated(sd, widths, rows, target, nv, mask, 0.125)
    assert got[2] == want[2] == int(is_live(nv, mask).sum())
    assert same_bytes(got[0], want[0]) and got[1] == want[1]
    live = is_live(nv, mask)
    assert same_bytes(got[4][live], want[4][live]) and same_bytes(got[3][live], want[3][live])
    # a chunk boundary is a boundary of nothing but the sums: the two chunks of 17 .. 32 states, each in a call of its own,
    # add up in float64 to the one call
    if 16 < B <= 32:
        a = host_grad(P, widths, rows[:16], target[:16], nv[:16], mask[:16], grad_scale=0.125)
        b = host_grad(P, widths, rows[16:], target[16:], nv[16:], mask[16:], grad_scale=0.125)
        assert same_bytes(got[0], (a[0].astype(np.float64) + b[0].astype(np.float64)).astype(np.float32))
        assert got[1] == a[1] + b[1] and got[2] == a[2] + b[2]


# ---------------------------------------------------------------------- the host program under the sanitizers
def test_host_program_runs_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, built with -fsanitize=address,undefined, over the edge batches of every B x R at the narrow
    widths and of two shapes at the reference widths: no finding, and the bytes of the library build."""
    batches = []
    for widths, shapes in ((NARROW_WIDTHS, [(B, R) for B in BATCHES for R in (1, 2, 5, 18)]), (REFERENCE_WIDTHS, [(17, 2), (1, 1)])):
        P = host_pack(random_state_dict(widths))
        for B, R in shapes:
            rows, target, nv, mask, _ = edge_batch(widths, B, R)
            batches.append((widths, P, rows, target, nv, mask, 2.0 / B))
    rows, target = plain_batch(NARROW_WIDTHS, 3, 2, seed=67)
    batches.append((NARROW_WIDTHS, batches[0][1], rows, target, None, None, 1.0))
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_batches(src, batches)
    done = subprocess.run([host_program(sanitize=True), src, out], check=True, capture_output=True, text=True, timeout=600)
    assert "cadrl_grad_host: %d batches" % len(batches) in done.stdout and "runtime error" not in done.stderr, done.stderr
    for (widths, P, rows, target, nv, mask, scale), got in zip(batches, read_results(out, batches)):
        want = host_grad(P, widths, rows, target, nv, mask, scale)
        assert same_bytes(got[0], want[0]) and np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes() and got[2] == want[2]
        assert same_bytes(got[3], want[3]) and same_bytes(got[4], want[4])


# ---------------------------------------------------------------------- the reference's Trainer steps
def _torch_steps(z, dtype):
    """The golden's three SGD steps restated with plain torch in `dtype`: (losses, the parameters after each step)."""
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0_")}
    m = CadrlModule.from_state_dict(sd).to(dtype)
    opt = torch.optim.SGD(m.parameters(), lr=float(z["lr"]), momentum=0.9)
    losses, after = [], []
    for a, b in z["batches"]:
        opt.zero_grad()
        out = m.value_network(torch.from_numpy(z["states"][a:b]).to(dtype))
        loss = torch.nn.functional.mse_loss(out, torch.from_numpy(z["values"][a:b]).to(dtype)[:, None])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        after.append({k: v.detach().double().numpy().copy() for k, v in m.state_dict().items()})
    return losses, after


def test_trainer_reproduces_the_reference_trainer_steps():
    """Three SGD steps of the reference's own Trainer.optimize_batch on R = 1 states of the cadrl_one run (the golden):
    CadrlTrainer(native=False) on the CPU gives its losses and its weights after each step within TOL_FACTOR times torch's
    own float32 error against the same steps in float64 (measured here, per step and per tensor)."""
    z = load("cadrl_one_trainer_steps")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p0_")}
    assert list(sd) == [k + s for k in LAYER_KEYS for s in (".weight", ".bias")]
    l32, w32 = _torch_steps(z, torch.float32)
    l64, w64 = _torch_steps(z, torch.float64)
    tr = CadrlTrainer(sd, device="cpu", optimizer="sgd", lr=float(z["lr"]), native=False)
    assert tr.native is False and tr.flat.is_leaf and tr.flat.requires_grad
    for i, (a, b) in enumerate(z["batches"]):
        loss, count = tr.loss_and_grad(torch.from_numpy(z["states"][a:b])[:, None, :], torch.from_numpy(z["values"][a:b]))
        tr.step()
        mse = float(loss) / int(count)
        tol = TOL_FACTOR * abs(l32[i] - l64[i])
        print("step %d loss %.9g golden %.9g torch32 error %.3e" % (i, mse, float(z["loss"][i]), abs(l32[i] - l64[i])))
        assert int(count) == b - a and tol > 0 and abs(mse - float(z["loss"][i])) <= tol
        got = tr.state_dict()
        for k in sd:
            e_ref = float(np.abs(w32[i][k] - w64[i][k]).max())
            err = float(np.abs(got[k].numpy().astype(np.float64) - z["p%d_%s" % (i + 1, k)]).max())
            assert e_ref > 0 and err <= TOL_FACTOR * e_ref, (i, k, err, e_ref)
    assert not torch.equal(tr.state_dict()[LAYER_KEYS[0] + ".weight"], sd[LAYER_KEYS[0] + ".weight"])


def test_saved_file_loads_strict_and_refreshes_a_value_net(tmp_path):
    widths = NARROW_WIDTHS
    sd = random_state_dict(widths)
    tr = CadrlTrainer(sd, device="cpu", optimizer="adam", lr=1e-3)
    rows, target, nv, mask, _ = edge_batch(widths, 19, 3, seed=68)
    loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
    assert int(count) == int(is_live(nv, mask).sum()) and bool(torch.isfinite(tr.flat.grad).all()) and np.isfinite(float(loss))
    tr.step()
    path = str(tmp_path / "cadrl_model.pth")
    tr.save(path)
    loaded = torch.load(path, map_location="cpu")
    CadrlModule(widths[0], widths[1:]).load_state_dict(loaded, strict=True)
    assert list(loaded) == list(sd) and not all(torch.equal(loaded[k], sd[k]) for k in sd)
    net, fresh = CadrlValueNet(sd), CadrlValueNet.load(path)
    assert net.refresh_native(tr) is False  # a CPU device has no blocks; the module has the weights
    x = torch.from_numpy(plain_batch(widths, 7, 3, seed=69)[0])
    assert torch.equal(net.forward(x), fresh.forward(x))
    pad = pack_state_dict({k: torch.ones_like(v) for k, v in sd.items()}) == 0
    assert bool((tr.flat.detach()[pad] == 0).all()) and bool((tr.flat.grad[pad] == 0).all())
    with pytest.raises(NotImplementedError):
        CadrlTrainer(sd, device="cpu", native=True)


def test_autograd_path_against_the_host_build():
    """CadrlTrainer(native=False) over an edge batch: count, loss and gradient agree with the rule's host build to float32
    rounding (two float32 evaluations of the same sums)."""
    widths, sd, P = _net()
    rows, target, nv, mask, _ = edge_batch(widths, 33, 5, seed=71)
    tr = CadrlTrainer(sd, device="cpu", native=False)
    loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
    live = is_live(nv, mask)
    g, hl, hc, _, _ = host_grad(P, widths, rows, target, nv, mask, 2.0 / live.sum())
    assert int(count) == hc == int(live.sum()) and abs(float(loss) - hl) <= 1e-5 * hl
    np.testing.assert_allclose(tr.flat.grad.numpy(), g, rtol=0, atol=2e-5 * np.abs(g).max())


def test_one_human_config_sets_every_reward_the_rollouts_can_meet():
    """configs/cadrl_one_human.config through the schema's reader: the four collision penalties and the success reward
    are finite (a penalty the config does not set is NaN, and the first collision of an exploring robot then poisons the
    value targets), one adult, no static rows; and the schedule's guard raises on anything that is not finite."""
    import configparser
    from ebcsim import config as ebc_config, scene as ebc_scene
    from ebcsim.cadrl_train import _finite
    cfg, pol = configparser.RawConfigParser(), configparser.RawConfigParser()
    cfg.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "cadrl_one_human.config"))
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_plain.config"))
    params = ebc_config.params_from_config(cfg, pol, policy="cadrl")
    assert [float(v) for v in params.collision_penalty] == [-0.25] * 4 and params.success_reward == 1.0 and params.with_agent_type == 0
    sc = ebc_scene.SceneConfig.from_config(cfg)
    assert list(ebc_scene.gen_struct(sc, "train").count) == [1, 0, 0] and ebc_scene.max_static_rows(sc) == 0

    class Env(object):
        pass
    Env.params = params
    _finite(0.5, "x", Env)
    _finite(torch.zeros(3), "x", Env)
    for bad in (float("nan"), float("inf"), torch.tensor([0.0, float("nan")])):
        with pytest.raises(FloatingPointError):
            _finite(bad, "x", Env)


# ---------------------------------------------------------------------- the C ABI
NEW_ENTRIES = (("ebc_cadrl_net_create", 3), ("ebc_cadrl_net_destroy", 1), ("ebc_cadrl_net_packed_floats", 2), ("ebc_cadrl_net_get_packed", 3),
               ("ebc_cadrl_net_set_packed", 3), ("ebc_cadrl_grad", 3))


def test_bindings_match_the_header():
    text = open(HEADER).read()
    names = re.findall(r"^(?:int|const char \*)\s*(ebc_\w+)\(", text, flags=re.M)
    assert set(names) == set(_capi.SYMBOLS) and len(names) == len(set(names))
    assert _abi.ABI_VERSION == 1 and re.search(r"#define EBC_ABI_VERSION 1\b", text)
    for name, n_args in NEW_ENTRIES:
        m = re.search(r"int %s\(([^)]*)\);" % name, text)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int


@pytest.mark.parametrize("name", ["EbcCadrlNetWeights", "EbcCadrlGradArgs"])
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
