"""Training SARL without a GPU: the host build of the gradient rule (csrc/ebc_sarl_grad_rule.h) against torch's autograd of
SarlModule, its edges stated one by one (rows past n_valid, row counts of 0, below 0 and above R, masked states, a batch
without a live state, a NaN in a live row, a score of exactly 0, R = 1, no global state), the chunk sums against a plain
restatement, the host program under the sanitizers, the reference's own Trainer steps
(tests/golden/sarl_a5_trainer_steps.npz) and the C ABI's declarations.  Cases and the bar: tests/sarl_grad_cases.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sarl_grad_cases import (BATCHES, NARROW_LOCAL_NET, NARROW_NET, NARROW_T17_NET, NETS, REFERENCE_NET, ROWS, TOL_FACTOR, accuracy_cases,
                             accuracy_row, batches, chunk, edge_batch, host_floats, host_grad, host_layers, host_pack, host_program,
                             is_live, layer_slices, module, plain_batch, random_state_dict, read_results, same_bytes, torch_grad,
                             torch_scores, write_batches)
from helpers import GOLDEN, load
from ebcsim import _abi, _capi
from ebcsim.sarl_train import (LAYER_KEYS, SarlTrainer, layer_inputs, pack_state_dict, packed_floats, shape_of, unpack_to_state_dict,
                               widths_of)
from ebcsim.train import SarlModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")
NAN32, NAN64 = 0x7fc00000, 0x7ff8000000000000


@pytest.mark.parametrize("ni,B,R", accuracy_cases())
def test_host_build_against_float64_autograd(ni, B, R):
    """Per layer and for the loss: the rule's error against float64 autograd is within TOL_FACTOR times the error of
    torch's own float32 autograd on the same weights and inputs.  Precondition: in float64 no score is exactly 0 and no
    softmax denominator is 0."""
    layers, (loss_rule, loss_t32), (min_score, min_den), seed = accuracy_row(ni, B, R)
    for name, err_rule, err_t32 in layers + [("loss_sum", loss_rule, loss_t32)]:
        print("net %d B %3d R %2d seed %d %-14s rule %.3e torch32 %.3e" % (ni, B, R, seed, name, err_rule, err_t32))
    assert min_score > 0 and min_den > 0, (min_score, min_den)
    for name, err_rule, err_t32 in layers:
        assert err_rule <= TOL_FACTOR * err_t32, (name, err_rule, err_t32)
    assert loss_rule <= TOL_FACTOR * loss_t32, (loss_rule, loss_t32)


def test_packed_layout_is_the_documented_one():
    """W[k][units padded to a multiple of 4] then the bias, layer after layer in the order mlp1, mlp2, attention, mlp3;
    97 452 floats at the reference widths; the python packer, the header's packer and unpack agree; pad entries are 0."""
    assert batches() == BATCHES and ROWS == [1, 2, 5, 10]
    assert host_floats(REFERENCE_NET) == packed_floats(*REFERENCE_NET) == 97452
    assert [op for _, _, op in host_layers(REFERENCE_NET)] == [152, 100, 100, 52, 100, 100, 4, 152, 100, 100, 4]
    assert [k for _, k, _ in host_layers(REFERENCE_NET)] == [13, 150, 100, 100, 200, 100, 100, 56, 150, 100, 100]
    assert LAYER_KEYS == ("mlp1.0", "mlp1.2", "mlp2.0", "mlp2.2", "attention.0", "attention.2", "attention.4", "mlp3.0", "mlp3.2",
                          "mlp3.4", "mlp3.6")
    for net in NETS:
        sd = random_state_dict(net)
        assert shape_of(sd) == (net[0], net[1], net[2]) and widths_of(sd) == net[0]
        flat = pack_state_dict(sd)
        assert same_bytes(flat.numpy(), host_pack(sd)) and flat.numel() == host_floats(net)
        at = 0
        for k, o, key, (off, kk, op) in zip(layer_inputs(*net), net[0][1:], LAYER_KEYS, host_layers(net)):
            assert off == at and op == (o + 3) // 4 * 4 and kk == k
            W = flat[at:at + k * op].view(k, op)
            assert torch.equal(W[:, :o], sd[key + ".weight"].t()) and bool((W[:, o:] == 0).all())
            assert torch.equal(flat[at + k * op:at + k * op + o], sd[key + ".bias"]) and bool((flat[at + k * op + o:at + (k + 1) * op] == 0).all())
            at += (k + 1) * op
        back = unpack_to_state_dict(flat, *net)
        assert list(back) == list(module(net).state_dict()) and all(torch.equal(back[k], sd[k]) for k in sd)
        # pad entries of the gradient are 0 too
        rows, target = plain_batch(net, 5, 3, seed=80)
        g = host_grad(host_pack(sd), net, rows, target)[0]
        pad = pack_state_dict({k: torch.ones_like(v) for k, v in sd.items()}).numpy() == 0
        assert pad.sum() > 0 and (g[pad].view(np.uint32) == 0).all() and np.abs(g[~pad]).max() > 0


# ---------------------------------------------------------------------- edge states, one by one
def _net(net=NARROW_NET):
    sd = random_state_dict(net)
    return net, sd, host_pack(sd)


def _same(a, b, live=None):
    ok = same_bytes(a[0], b[0]) and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes() and a[2] == b[2]
    if live is None:
        return ok and same_bytes(a[3], b[3]) and same_bytes(a[4], b[4])
    return ok and same_bytes(a[3][live], b[3][live]) and same_bytes(a[4][live], b[4][live])


def test_rows_past_n_valid_reach_nothing():
    """NaN and both infinities in the rows at or past n_valid: value, gradient, loss and attention weights have the bytes of
    the same batch with zeros there, and of the batch cut to the valid rows where every state has the same count; the
    attention weights past n_valid are 0."""
    net, sd, P = _net()
    B, R = chunk() + 3, 5
    rows, target = plain_batch(net, B, R, seed=62)
    nv = np.array([1 + b % (R - 1) for b in range(B)], dtype=np.int64)
    clean = rows.copy()
    for b in range(B):
        for r in range(int(nv[b]), R):
            rows[b, r] = (np.nan, np.inf, -np.inf)[(r + b) % 3]
            clean[b, r] = 0.0
    bad, good = host_grad(P, net, rows, target, nv, grad_scale=2.0 / B), host_grad(P, net, clean, target, nv, grad_scale=2.0 / B)
    assert np.isfinite(bad[0]).all() and np.abs(bad[0]).max() > 0 and np.isfinite(bad[1]) and bad[2] == B
    assert _same(bad, good) and np.isfinite(bad[3]).all() and np.isfinite(bad[4]).all()
    past = np.arange(R)[None, :] >= nv[:, None]
    assert (bad[4][past].view(np.uint32) == 0).all() and (bad[4][~past] > 0).all()
    np.testing.assert_allclose(bad[4].sum(1), 1.0, atol=1e-6)
    two = np.full(B, 2, dtype=np.int64)
    rows = clean.copy()
    rows[:, 2:] = np.nan
    cut = host_grad(P, net, np.ascontiguousarray(rows[:, :2]), target, None, grad_scale=2.0 / B)
    full = host_grad(P, net, rows, target, two, grad_scale=2.0 / B)
    assert np.isfinite(cut[0]).all() and same_bytes(cut[0], full[0]) and cut[1] == full[1] and same_bytes(cut[3], full[3])
    assert same_bytes(cut[4], full[4][:, :2])


def test_n_valid_of_zero_is_not_live():
    net, sd, P = _net()
    rows, target = plain_batch(net, 3, 3, seed=63)
    nv = np.array([3, 0, 3], dtype=np.int64)
    poisoned = rows.copy()
    poisoned[1] = np.nan  # a state without rows reads none of them
    got = host_grad(P, net, poisoned, target, nv, grad_scale=1.0)
    assert got[2] == 2 and np.isfinite(got[0]).all() and np.isfinite(got[1])
    assert got[3][1:2].view(np.uint32)[0] == NAN32 and (got[4][1].view(np.uint32) == 0).all()
    want = host_grad(P, net, rows[[0, 2]], target[[0, 2]], None, grad_scale=1.0)
    assert same_bytes(got[0], want[0]) and got[1] == want[1] and same_bytes(got[3][[0, 2]], want[3]) and same_bytes(got[4][[0, 2]], want[4])


def test_negative_n_valid_is_not_live():
    net, sd, P = _net()
    rows, target = plain_batch(net, 3, 3, seed=64)
    poisoned = rows.copy()
    poisoned[0] = np.nan
    got = host_grad(P, net, poisoned, target, np.array([-5, 3, 3], dtype=np.int64), grad_scale=1.0)
    want = host_grad(P, net, rows[1:], target[1:], None, grad_scale=1.0)
    assert got[2] == 2 and got[3][:1].view(np.uint32)[0] == NAN32 and (got[4][0].view(np.uint32) == 0).all()
    assert same_bytes(got[0], want[0]) and got[1] == want[1] and same_bytes(got[3][1:], want[3]) and same_bytes(got[4][1:], want[4])


def test_n_valid_above_r_is_clamped():
    net, sd, P = _net()
    rows, target = plain_batch(net, 3, 3, seed=65)
    got = host_grad(P, net, rows, target, np.array([3 + 7, 3, 1 << 40], dtype=np.int64), grad_scale=1.0)
    assert _same(got, host_grad(P, net, rows, target, None, grad_scale=1.0)) and got[2] == 3


def test_a_masked_state_enters_no_sum():
    net, sd, P = _net()
    B = chunk() + 5
    rows, target = plain_batch(net, B, 2, seed=66)
    mask = np.array([b % 3 != 1 for b in range(B)], dtype=np.uint8)
    poisoned, ptarget = rows.copy(), target.copy()
    poisoned[mask == 0, 1, 4] = np.nan
    poisoned[mask == 0, 0, 0] = np.inf
    ptarget[mask == 0] = np.nan
    a, b = host_grad(P, net, poisoned, ptarget, None, mask, grad_scale=0.25), host_grad(P, net, rows, target, None, mask, grad_scale=0.25)
    assert np.isfinite(a[0]).all() and _same(a, b, mask != 0) and a[2] == int(mask.sum())
    assert (a[3][mask == 0].view(np.uint32) == NAN32).all()
    # against float64 autograd of the live states alone
    g64, l64, _ = torch_grad(sd, rows, target, None, mask != 0, 0.25, torch.float64)
    np.testing.assert_allclose(a[0], g64, rtol=0, atol=2e-5 * np.abs(g64).max())
    assert abs(a[1] - l64) <= 1e-5 * l64


def test_a_batch_with_no_live_state():
    net, sd, P = _net()
    B = chunk() + 2
    rows, target = plain_batch(net, B, 3, seed=67)
    for kw in (dict(mask=np.zeros(B, np.uint8)), dict(n_valid=np.zeros(B, np.int64)), dict(n_valid=np.full(B, -1, np.int64))):
        g, loss, count, value, att = host_grad(P, net, rows, target, grad_scale=0.5, **kw)
        assert count == 0 and loss == 0.0 and (g.view(np.uint32) == 0).all()
    g, loss, count, _, _ = host_grad(P, net, rows[:0], target[:0])
    assert count == 0 and loss == 0.0 and (g.view(np.uint32) == 0).all()


def test_a_nan_in_a_live_row_reaches_the_loss_and_the_gradient():
    net, sd, P = _net()
    rows, target = plain_batch(net, 5, 2, seed=68)
    rows[3, 1, 7] = np.nan
    g, loss, count, value, att = host_grad(P, net, rows, target, grad_scale=0.4)
    assert count == 5 and np.isnan(loss) and np.float64(loss).view(np.uint64) == NAN64
    assert value[3:4].view(np.uint32)[0] == NAN32 and np.isfinite(np.delete(value, 3)).all()
    assert np.isnan(g).any() and (g[np.isnan(g)].view(np.uint32) == NAN32).all()
    assert (att[3][np.isnan(att[3])].view(np.uint32) == NAN32).all() and np.isnan(att[3]).any() and np.isfinite(np.delete(att, 3, 0)).all()
    s = layer_slices(net)[10]
    assert np.isnan(g[s][:net[0][10] * 4:4]).all()  # mlp3's last layer: the seed times the kept activations


def test_a_score_of_exactly_zero_gets_weight_zero_and_passes_nothing_on():
    """attention's last layer zeroed, with a zero bias, but for ONE weight of 1: a row's score is that ReLU output, exactly
    0 where the ReLU is dead.  Such a row gets weight 0 and the gradient agrees with float64 autograd of the reference's
    formula, in which exp(s) * (s != 0) passes nothing on at 0.  With the layer zeroed altogether every score is 0 and the
    weights are the reference's 0 / 0: NaN."""
    net = NARROW_NET
    sd = random_state_dict(net)
    sd = {k: v.clone() for k, v in sd.items()}
    # scores = c2[u0]: the last layer keeps ONE weight of 1 on a unit u0 that is live with torch's initialisation, and that
    # unit's bias is lowered by the median of its float64 outputs over the batch, so about half of the rows die
    u0 = 3
    w = torch.zeros_like(sd["attention.4.weight"])
    w[0, u0] = 1.0
    sd["attention.4.weight"], sd["attention.4.bias"] = w, torch.zeros_like(sd["attention.4.bias"])
    rows, target = None, None
    for seed in range(200):
        r, t = plain_batch(net, 6, 5, seed=900 + seed)
        s64, _, _, _ = torch_scores(sd, r, None, torch.float64)
        assert (s64 > 0).all()
        trial = dict(sd)
        trial["attention.2.bias"] = sd["attention.2.bias"].clone()
        trial["attention.2.bias"][u0] -= float(np.median(s64))
        s64, den64, _, _ = torch_scores(trial, r, None, torch.float64)
        s32, _, _, _ = torch_scores(trial, r, None, torch.float32)
        zero = s64 == 0
        if zero.any() and (~zero).any(1).all() and ((s32 == 0) == zero).all() and (den64 > 0).all():
            rows, target, sd = r, t, trial
            break
    assert rows is not None, "no seed gives a dead row and every state a live one"
    P = host_pack(sd)
    g, loss, count, value, att = host_grad(P, net, rows, target, grad_scale=1.0)
    assert count == 6 and np.isfinite(g).all() and np.isfinite(value).all()
    assert (att[zero].view(np.uint32) == 0).all() and (att[~zero] > 0).all()
    np.testing.assert_allclose(att.sum(1), 1.0, atol=1e-6)
    # nothing of a zero-score row passes through the exponential: the batch with those rows' mlp2 features and scores
    # out of reach gives the same attention-stack gradient as float64 autograd of the reference's formula
    g64, l64, v64 = torch_grad(sd, rows, target, None, np.ones(6, dtype=bool), 1.0, torch.float64)
    np.testing.assert_allclose(g, g64, rtol=0, atol=2e-5 * np.abs(g64).max())
    np.testing.assert_allclose(value, v64, atol=1e-5)
    # and when EVERY score is 0 (the last layer zeroed altogether) the weights are the reference's 0 / 0
    sd["attention.4.weight"] = torch.zeros_like(w)
    g, loss, count, value, att = host_grad(host_pack(sd), net, rows, target, grad_scale=1.0)
    assert (att.view(np.uint32) == NAN32).all() and (value.view(np.uint32) == NAN32).all() and np.isnan(loss)


def test_one_row_gives_weight_one_and_no_gradient_to_attention():
    net, sd, P = _net()
    rows, target = plain_batch(net, chunk() + 1, 1, seed=69)
    g, loss, count, value, att = host_grad(P, net, rows, target, grad_scale=0.5)
    assert count == chunk() + 1 and (att == 1.0).all() and np.isfinite(g).all()
    s = layer_slices(net)
    for l in (4, 5, 6):
        assert (g[s[l]] == 0).all()
    for l in (0, 1, 2, 3, 7, 8, 9, 10):
        assert np.abs(g[s[l]]).max() > 0
    g64, l64, _ = torch_grad(sd, rows, target, None, np.ones(len(target), dtype=bool), 0.5, torch.float64)
    np.testing.assert_allclose(g, g64, rtol=0, atol=2e-5 * np.abs(g64).max())


@pytest.mark.parametrize("net", [NARROW_LOCAL_NET, NARROW_T17_NET], ids=["no_global_state", "rows_17_wide"])
def test_without_global_state_and_with_wide_rows(net):
    net, sd, P = _net(net)
    assert layer_inputs(*net)[4] == net[0][2] * (2 if net[2] else 1)
    rows, target, nv, mask, _ = edge_batch(net, 2 * chunk() + 1, 5, seed=70)
    live = is_live(nv, mask)
    g, loss, count, value, att = host_grad(P, net, rows, target, nv, mask, grad_scale=2.0 / live.sum())
    g64, l64, v64 = torch_grad(sd, rows, target, nv, live, 2.0 / live.sum(), torch.float64)
    assert count == int(live.sum()) and abs(loss - l64) <= 1e-5 * l64
    np.testing.assert_allclose(g, g64, rtol=0, atol=2e-5 * np.abs(g64).max())
    np.testing.assert_allclose(value[live], v64, atol=1e-5)


# ---------------------------------------------------------------------- chunking
_LD = np.longdouble  # 64 bits of mantissa: a float32 product is exact in it and a + of a float32 rounds far below float32's half spacing
f32 = np.float32


def _fma32(a, b, c):
    """fmaf on float32 arrays: the exact product plus c, rounded to float32 once."""
    return (np.asarray(a, dtype=f32).astype(_LD) * np.asarray(b, dtype=f32).astype(_LD) + np.asarray(c, dtype=f32).astype(_LD)).astype(f32)


def _exp32(s):
    """exp of a float32 score as csrc/ebc_lstm_cell.h: exp_parts builds it, on s clamped to [-87, 88]: sc * (1 + p)."""
    z = f32(min(max(float(s), -87.0), 88.0))
    magic = f32(12582912.0)
    t = _fma32(z, f32(1.44269504088896341), magic)
    n = f32(t - magic)
    r = _fma32(n, f32(-0.693145751953125), z)
    r = _fma32(n, f32(-1.42860682030941723e-6), r)
    q = f32(2.48015873015873016e-5)
    for c in (1.98412698412698413e-4, 1.38888888888888894e-3, 8.33333333333333322e-3, 4.16666666666666644e-2, 1.66666666666666657e-1, 0.5):
        q = _fma32(q, r, f32(c))
    p = _fma32(f32(q * r), r, r)
    sc = f32(2.0) ** f32(int(n))
    return _fma32(sc, p, sc)


def _restated(sd, net, rows, target, nv, mask, scale):
    """The rule in plain numpy, written from its text (the head of csrc/ebc_sarl_grad_rule.h): units as chains over their
    inputs ascending from 0 and then + bias, the mean, the masked softmax with float64 quotients, the weighted sum, the
    Linear and ReLU backward, the softmax's and the mean's backward, every weight's chain over a chunk's live states and
    their rows ascending from 0, the chunks of 4 added in float64 and rounded once; the loss in float64."""
    widths, S, glob = net
    W = [sd[k + ".weight"].numpy().T.astype(f32) for k in LAYER_KEYS]  # [K][O]
    bias = [sd[k + ".bias"].numpy().astype(f32) for k in LAYER_KEYS]
    H, F = widths[2], widths[4]

    def lin(l, x, relu):
        acc = np.zeros(W[l].shape[1], dtype=f32)
        for k in range(W[l].shape[0]):
            acc = _fma32(x[k], W[l][k], acc)
        y = acc + bias[l]
        return np.where(y < 0, f32(0), y) if relu else y

    def back(l, G, x, delta, want_dx=True):
        G[l] = (_fma32(delta[None, :], x[:, None], G[l][0]), G[l][1] + delta)
        if not want_dx:
            return None
        dx = np.zeros(W[l].shape[0], dtype=f32)
        for u in range(W[l].shape[1]):
            dx = _fma32(W[l][:, u], delta[u], dx)
        return dx

    def quot(a, b):
        return f32(np.float64(a) / np.float64(b))

    B, R, _ = rows.shape
    total = [(np.zeros(w.shape, np.float64), np.zeros(b.shape, np.float64)) for w, b in zip(W, bias)]
    loss, count, value, att = 0.0, 0, np.full(B, np.nan, dtype=f32), np.zeros((B, R), dtype=f32)
    for c0 in range(0, B, 4):
        G = [(np.zeros(w.shape, f32), np.zeros(b.shape, f32)) for w, b in zip(W, bias)]
        chunk_loss = 0.0
        for b in range(c0, min(B, c0 + 4)):
            n = R if nv is None else max(0, min(R, int(nv[b])))
            if n < 1 or (mask is not None and not mask[b]):
                continue  # not live: nothing of it is looked at
            x = [rows[b, r].astype(f32) for r in range(n)]
            a1 = [lin(0, x[r], True) for r in range(n)]
            h1 = [lin(1, a1[r], True) for r in range(n)]
            b1 = [lin(2, h1[r], True) for r in range(n)]
            ft = [lin(3, b1[r], False) for r in range(n)]
            xa = h1
            if glob:
                acc = np.zeros(H, dtype=f32)
                for r in range(n):
                    acc = acc + h1[r]
                g = (acc.astype(np.float64) / np.float64(n)).astype(f32)
                xa = [np.concatenate([h1[r], g]) for r in range(n)]
            c1 = [lin(4, xa[r], True) for r in range(n)]
            c2 = [lin(5, c1[r], True) for r in range(n)]
            s = [lin(6, c2[r], False)[0] for r in range(n)]
            assert all(np.isfinite(v) for v in s)
            e = [_exp32(v) if v != 0 else f32(0) for v in s]
            den = f32(0)
            for r in range(n):
                den = f32(den + e[r])
            w = [quot(e[r], den) for r in range(n)]
            wf = np.zeros(F, dtype=f32)
            for r in range(n):
                wf = _fma32(w[r], ft[r], wf)
            j = np.concatenate([x[0][:S], wf])
            m1 = lin(7, j, True)
            m2 = lin(8, m1, True)
            m3 = lin(9, m2, True)
            out = lin(10, m3, False)[0]
            value[b], att[b, :n] = out, w
            d = f32(out - f32(target[b]))
            chunk_loss, count = chunk_loss + float(d) * float(d), count + 1
            # backward
            d3 = np.where(m3 > 0, back(10, G, m3, np.array([f32(scale) * d], dtype=f32)), f32(0))
            d2 = np.where(m2 > 0, back(9, G, m2, d3), f32(0))
            d1 = np.where(m1 > 0, back(8, G, m1, d2), f32(0))
            dwf = back(7, G, j, d1)[S:]
            c = []
            for r in range(n):
                acc = f32(0)
                for f in range(F):
                    acc = _fma32(dwf[f], f32(ft[r][f] - wf[f]), acc)
                c.append(acc)
            m = f32(0)
            for r in range(n):
                m = _fma32(w[r], c[r], m)
            ds = [f32(w[r] * f32(c[r] - m)) for r in range(n)]
            dft = [(w[r] * dwf).astype(f32) for r in range(n)]
            db1 = [np.where(b1[r] > 0, back(3, G, b1[r], dft[r]), f32(0)) for r in range(n)]
            for r in range(n):
                back(2, G, h1[r], db1[r], False)
            dc2 = [np.where(c2[r] > 0, back(6, G, c2[r], np.array([ds[r]], dtype=f32)), f32(0)) for r in range(n)]
            dc1 = [np.where(c1[r] > 0, back(5, G, c1[r], dc2[r]), f32(0)) for r in range(n)]
            for r in range(n):
                back(4, G, xa[r], dc1[r], False)

            def dx_of(l, k, delta):
                acc = f32(0)
                for u in range(W[l].shape[1]):
                    acc = _fma32(W[l][k, u], delta[u], acc)
                return acc
            dm = np.zeros(H, dtype=f32)
            if glob:
                for k in range(H):
                    dg = f32(0)
                    for r in range(n):
                        dg = f32(dg + dx_of(4, H + k, dc1[r]))
                    dm[k] = quot(dg, n)
            dh1 = []
            for r in range(n):
                v = np.zeros(H, dtype=f32)
                for k in range(H):
                    t = f32(dx_of(2, k, db1[r]) + dx_of(4, k, dc1[r]))
                    if glob:
                        t = f32(t + dm[k])
                    v[k] = t if h1[r][k] > 0 else f32(0)
                dh1.append(v)
            da1 = [np.where(a1[r] > 0, back(1, G, a1[r], dh1[r]), f32(0)) for r in range(n)]
            for r in range(n):
                back(0, G, x[r], da1[r], False)
        total = [(tw + gw.astype(np.float64), tb + gb.astype(np.float64)) for (tw, tb), (gw, gb) in zip(total, G)]
        loss = loss + chunk_loss
    flat, at = np.zeros(packed_floats(*net), dtype=f32), 0
    for l, (tw, tb) in enumerate(total):
        K, O = tw.shape
        Op = (O + 3) // 4 * 4
        flat[at:at + K * Op].reshape(K, Op)[:, :O] = tw.astype(f32)
        flat[at + K * Op:at + K * Op + O] = tb.astype(f32)
        at += (K + 1) * Op
    return flat, loss, count, value, att


@pytest.mark.parametrize("net", [NARROW_NET, NARROW_LOCAL_NET], ids=["global_state", "no_global_state"])
def test_chunk_sums_against_a_plain_restatement(net):
    """B = 2 C + 1: the host build gives the bytes of the rule restated in numpy (chains and chunk sums written out in the
    test), on an edge batch: gradient, loss, count, values and attention weights."""
    assert chunk() == 4
    net, sd, P = _net(net)
    B = 2 * chunk() + 1
    rows, target, nv, mask, kinds = edge_batch(net, B, 3, seed=70 + B)
    got = host_grad(P, net, rows, target, nv, mask, grad_scale=0.125)
    want = _restated(sd, net, rows, target, nv, mask, 0.125)
    live = is_live(nv, mask)
    assert got[2] == want[2] == int(live.sum()) and live.sum() >= 4
    assert same_bytes(got[0], want[0]) and got[1] == want[1]
    assert same_bytes(got[3][live], want[3][live]) and same_bytes(got[4][live], want[4][live])
    # a chunk boundary is a boundary of nothing but the sums: the three chunks, each in a call of its own, add up in
    # float64 to the one call
    parts = [host_grad(P, net, rows[a:a + 4], target[a:a + 4], nv[a:a + 4], mask[a:a + 4], grad_scale=0.125) for a in (0, 4, 8)]
    acc = np.zeros(len(P), dtype=np.float64)
    for p in parts:
        acc = acc + p[0].astype(np.float64)
    assert same_bytes(got[0], acc.astype(np.float32)) and got[1] == (parts[0][1] + parts[1][1]) + parts[2][1] and got[2] == sum(p[2] for p in parts)


# ---------------------------------------------------------------------- the host program under the sanitizers
def test_host_program_runs_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, built with -fsanitize=address,undefined, over the edge batches of every B x R at the narrow
    widths (both values of with_global_state, both row widths) and of two shapes at the reference widths: no finding, and
    the bytes of the library build.  The program is a process of its own: nothing of it is loaded into this one."""
    batch_list = []
    for net, shapes in ((NARROW_NET, [(B, R) for B in BATCHES for R in ROWS]), (NARROW_LOCAL_NET, [(9, 5), (1, 1)]),
                        (NARROW_T17_NET, [(5, 2)]), (REFERENCE_NET, [(5, 2), (1, 10)])):
        P = host_pack(random_state_dict(net))
        for B, R in shapes:
            rows, target, nv, mask, _ = edge_batch(net, B, R)
            batch_list.append((net, P, rows, target, nv, mask, 2.0 / B))
    rows, target = plain_batch(NARROW_NET, 3, 2, seed=67)
    batch_list.append((NARROW_NET, batch_list[0][1], rows, target, None, None, 1.0))
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_batches(src, batch_list)
    done = subprocess.run([host_program(sanitize=True), src, out], check=True, capture_output=True, text=True, timeout=600)
    assert "sarl_grad_host: %d batches" % len(batch_list) in done.stdout and "runtime error" not in done.stderr, done.stderr
    assert "Sanitizer" not in done.stderr, done.stderr
    for (net, P, rows, target, nv, mask, scale), got in zip(batch_list, read_results(out, batch_list)):
        assert _same(got, host_grad(P, net, rows, target, nv, mask, scale))


# ---------------------------------------------------------------------- the reference's Trainer steps
def test_autograd_trainer_reproduces_the_reference_trainer_steps():
    """Three SGD (momentum 0.9) steps of the reference's own Trainer on the 85 states of the golden RL memory, from the
    shipped a5 weights: SarlTrainer(native=False) on the CPU gives its losses and every parameter afterwards within the
    bars tests/test_train_gloo.py holds DataParallelTrainer to on the same golden."""
    g, t = load("sarl_a5_rl_memory"), load("sarl_a5_trainer_steps")
    sd = torch.load(os.path.join(GOLDEN, "weights", "sarl_a5_baseline.pth"), map_location="cpu")
    tr = SarlTrainer(sd, device="cpu", optimizer="sgd", lr=float(t["lr"]), native=False)
    assert tr.native is False and tr.flat.is_leaf and tr.flat.requires_grad and tr.widths == REFERENCE_NET[0] and tr.with_global_state
    states, values = torch.from_numpy(g["rl_state"]), torch.from_numpy(g["rl_value"])
    assert states.shape == (85, 5, 13)
    losses = []
    for _ in range(int(t["steps"])):
        loss, count = tr.loss_and_grad(states, values)
        tr.step()
        assert int(count) == 85
        losses.append(float(loss) / int(count))
    print("losses", losses, "golden", list(t["loss"]))
    np.testing.assert_allclose(losses, t["loss"], rtol=2e-5)
    after = tr.state_dict()
    assert list(after) == list(sd)
    for k in sd:
        np.testing.assert_allclose(after[k].numpy(), t["p_" + k], atol=2e-7, rtol=2e-5, err_msg=k)
        assert not np.array_equal(t["p_" + k], sd[k].numpy()) or k.endswith("bias")  # the steps moved the weights
    assert not torch.equal(after["mlp1.0.weight"], sd["mlp1.0.weight"])


def test_saved_file_loads_strict(tmp_path):
    net = NARROW_NET
    sd = random_state_dict(net)
    tr = SarlTrainer(sd, device="cpu", optimizer="adam", lr=1e-3)
    rows, target, nv, mask, _ = edge_batch(net, 11, 3, seed=68)
    loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
    assert int(count) == int(is_live(nv, mask).sum()) and bool(torch.isfinite(tr.flat.grad).all()) and np.isfinite(float(loss))
    tr.step()
    path = str(tmp_path / "sarl_model.pth")
    tr.save(path)
    loaded = torch.load(path, map_location="cpu")
    module(net).load_state_dict(loaded, strict=True)
    assert list(loaded) == list(sd) and not all(torch.equal(loaded[k], sd[k]) for k in sd)
    pad = pack_state_dict({k: torch.ones_like(v) for k, v in sd.items()}) == 0
    assert bool((tr.flat.detach()[pad] == 0).all()) and bool((tr.flat.grad[pad] == 0).all())
    with pytest.raises(NotImplementedError):
        SarlTrainer(sd, device="cpu", native=True)
    # a value network on the CPU takes the trainer's weights (no blocks there: refresh_from returns False)
    from ebcsim.sarl import SarlValueNet
    vn, fresh = SarlValueNet(sd, with_global_state=net[2], self_state_dim=net[1]), SarlValueNet.load(path, with_global_state=net[2], self_state_dim=net[1])
    assert vn.refresh_from(tr) is False
    x = torch.from_numpy(plain_batch(net, 7, 3, seed=69)[0])
    assert torch.equal(vn.forward(x), fresh.forward(x))


def test_autograd_path_against_the_host_build():
    """SarlTrainer(native=False) over an edge batch: count, loss and gradient agree with the rule's host build to float32
    rounding (two float32 evaluations of the same sums)."""
    net, sd, P = _net()
    rows, target, nv, mask, _ = edge_batch(net, 9, 5, seed=71)
    tr = SarlTrainer(sd, device="cpu", native=False)
    loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), torch.from_numpy(nv), torch.from_numpy(mask))
    live = is_live(nv, mask)
    g, hl, hc, _, _ = host_grad(P, net, rows, target, nv, mask, 2.0 / live.sum())
    assert int(count) == hc == int(live.sum()) and abs(float(loss) - hl) <= 1e-5 * hl
    np.testing.assert_allclose(tr.flat.grad.numpy(), g, rtol=0, atol=2e-5 * np.abs(g).max())


# ---------------------------------------------------------------------- the C ABI
NEW_ENTRIES = (("ebc_sarl_net_create", 3), ("ebc_sarl_net_destroy", 1), ("ebc_sarl_net_packed_floats", 2), ("ebc_sarl_net_get_packed", 3),
               ("ebc_sarl_net_set_packed", 3), ("ebc_sarl_net_grad_max_rows", 2), ("ebc_sarl_grad", 3))


def test_bindings_match_the_header():
    text = open(HEADER).read()
    names = re.findall(r"^(?:int|const char \*)\s*(ebc_\w+)\(", text, flags=re.M)
    assert set(names) == set(_capi.SYMBOLS) and len(names) == len(set(names))
    for name, n_args in NEW_ENTRIES:
        m = re.search(r"int %s\(([^)]*)\);" % name, text)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int


@pytest.mark.parametrize("name", ["EbcSarlNetWeights", "EbcSarlGradArgs"])
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
