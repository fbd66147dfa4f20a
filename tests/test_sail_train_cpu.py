"""Training SAIL without a GPU: the host build of the gradient rule (csrc/ebc_sail_grad_rule.h) against torch's autograd of
SailModule, its edges (a ReLU at exactly 0, masked envs with NaN, padding rows, pad entries), and the plumbing of
ebcsim.sail_train (packing, the saved file, the autograd path, the C ABI's declarations, a small fit).  Cases and the bar:
tests/sail_grad_cases.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sail_cases import random_state_dict, same_bytes
from sail_grad_cases import (TOL_FACTOR, accuracy_cases, accuracy_row, chunk, group, host_grad, host_pack, host_program, layer_slices,
                             masked_batch, plain_batch, torch_grad)
from ebcsim import _abi, _capi
from ebcsim.sail import LAYERS, SailModule, SailNet
from ebcsim.sail_train import SailTrainer, fit, layer_shapes, pack_state_dict, packed_floats, unpack_to_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")


@pytest.mark.parametrize("N,E", accuracy_cases())
def test_host_build_against_float64_autograd(N, E):
    """Per layer and for the loss: the rule's error against float64 autograd is within TOL_FACTOR times the error of
    torch's own float32 autograd on the same weights and inputs."""
    layers, (loss_rule, loss_t32) = accuracy_row(N, E)
    for name, err_rule, err_t32 in layers:
        print("N %2d E %3d %-18s rule %.3e torch32 %.3e" % (N, E, name, err_rule, err_t32))
    print("N %2d E %3d %-18s rule %.3e torch32 %.3e" % (N, E, "loss_sum", loss_rule, loss_t32))
    for name, err_rule, err_t32 in layers:
        assert err_rule <= TOL_FACTOR * err_t32, (N, E, name, err_rule, err_t32)
    assert loss_rule <= TOL_FACTOR * loss_t32, (N, E, loss_rule, loss_t32)


def test_chunk_and_group_constants():
    Cn = chunk()
    assert Cn >= 1
    for N in (2, 3, 5, 9, 32):
        assert 1 <= group(N) <= 8 and (group(N) == 1 or group(N) * N <= 32)


def test_relu_at_exactly_zero_passes_no_gradient():
    """joint_encoder's unit 0 with zero weights and zero bias has the pre-activation exactly 0: nothing flows into its
    weights or bias although the planner's weights on it are not 0, and torch agrees."""
    N, E = 5, 7
    sd = {k: v.clone() for k, v in random_state_dict(N, 8).items()}
    sd["joint_encoder.0.weight"][0] = 0.0
    sd["joint_encoder.0.bias"][0] = 0.0
    assert float(sd["planner.weight"][:, 0].abs().min()) > 0
    robot, ob, target = plain_batch(N, E, N, 41)
    g, loss, count, _ = host_grad(host_pack(sd), N, robot, ob, target, grad_scale=1.0 / E)
    s = layer_slices(N)[LAYERS.index("joint_encoder.0")]
    layer = g[s].reshape(129, 64)
    assert count == E and (layer[:, 0].view(np.int32) == 0).all() and np.abs(layer[:, 1:]).max() > 0
    g64, _ = torch_grad(sd, robot, ob, target, np.ones(E, bool), 1.0 / E, torch.float64)
    assert (g64[s].reshape(129, 64)[:, 0] == 0).all()
    np.testing.assert_allclose(g, g64, rtol=0, atol=2e-5 * np.abs(g64).max())


def test_a_batch_of_only_masked_envs():
    N, E = 3, chunk() + 2
    P = host_pack(random_state_dict(N, 8))
    robot, ob, target = plain_batch(N, E, N + 1, 42)
    for kw in (dict(mask=np.zeros(E, np.uint8)), dict(n_rows=np.full(E, N + 1, np.int64))):
        g, loss, count, action = host_grad(P, N, robot, ob, target, grad_scale=0.5, **kw)
        assert (g.view(np.int32) == 0).all() and loss == 0.0 and count == 0
    g, loss, count, _ = host_grad(P, N, robot[:0], ob[:0], target[:0])
    assert (g.view(np.int32) == 0).all() and loss == 0.0 and count == 0


@pytest.mark.parametrize("N", [2, 5])
def test_masked_envs_with_nan_reach_nothing(N):
    """Envs that do not count (masked out, ragged, arrived) full of NaN and infinities: the gradient is finite and has
    the bytes of the same batch with ordinary values there; so have the loss and the count; the live envs' actions too."""
    E, R = 2 * chunk() + 3, N + 2
    P = host_pack(random_state_dict(N, 8))
    bad = masked_batch(N, E, R, 43, poison=True)
    good = masked_batch(N, E, R, 43, poison=False)
    live = bad[5]
    assert (bad[3] == good[3]).all() and (bad[4] == good[4]).all() and not np.isfinite(bad[0][~live]).all()
    gb, lb, cb, ab = host_grad(P, N, bad[0], bad[1], bad[2], bad[3], bad[4], grad_scale=1.0 / live.sum())
    gg, lg, cg, ag = host_grad(P, N, good[0], good[1], good[2], good[3], good[4], grad_scale=1.0 / live.sum())
    assert np.isfinite(gb).all() and np.abs(gb).max() > 0 and same_bytes(gb, gg)
    assert lb == lg and np.isfinite(lb) and cb == cg == int(live.sum())
    assert same_bytes(ab[live], ag[live])
    # and the live envs alone, in the same chunks: what the masked ones add is nothing
    g64, l64 = torch_grad(random_state_dict(N, 8), good[0], good[1], good[2], live, 1.0 / live.sum(), torch.float64)
    np.testing.assert_allclose(gb, g64, rtol=0, atol=2e-5 * np.abs(g64).max())
    assert abs(lb - l64) <= 1e-5 * l64


def test_rows_past_adult_num_reach_nothing_and_pads_are_zero():
    N, E = 5, chunk() + 1
    sd = random_state_dict(N, 8)
    P = host_pack(sd)
    robot, ob, target = plain_batch(N, E, N + 3, 44)
    assert np.isnan(ob[:, N:]).any()
    clean = ob.copy()
    clean[:, N:] = 0.0
    g, loss, count, action = host_grad(P, N, robot, ob, target, grad_scale=1.0 / E)
    g2, loss2, count2, action2 = host_grad(P, N, robot, clean, target, grad_scale=1.0 / E)
    g3, loss3, _, _ = host_grad(P, N, robot, np.ascontiguousarray(ob[:, :N]), target, grad_scale=1.0 / E)
    assert np.isfinite(g).all() and same_bytes(g, g2) and same_bytes(g, g3) and loss == loss2 == loss3 and count == count2 == E
    assert same_bytes(action, action2)
    pad = pack_state_dict({k: torch.ones_like(v) for k, v in sd.items()}).numpy() == 0
    assert pad.sum() == packed_floats(N) - sum(k * o + o for k, o in layer_shapes(N))
    assert (g.view(np.int32)[pad] == 0).all() and (g[~pad] != 0).any()


def test_action_is_the_forward_of_the_host_build():
    from sail_cases import edge_batch, host_forward
    N = 5
    sd = random_state_dict(N, 8)
    robot, ob, n_rows, _ = edge_batch(N, 2 * chunk() + 3, N + 3)
    target = np.zeros((len(robot), 2))
    _, _, _, action = host_grad(host_pack(sd), N, robot, ob, target, n_rows=n_rows)
    assert same_bytes(action, host_forward(sd, robot, ob, n_rows)[0])


def test_host_program_runs_clean_under_the_sanitizers():
    out = subprocess.run([host_program(sanitize=True), "5", str(2 * chunk() + 3)], check=True, capture_output=True, text=True, timeout=300)
    assert "finite 1" in out.stdout, out.stdout
    plain = subprocess.run([host_program(), "5", str(2 * chunk() + 3)], check=True, capture_output=True, text=True, timeout=300)
    assert plain.stdout == out.stdout


# ---------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("N", [2, 5, 32])
def test_pack_and_unpack_are_inverse(N):
    sd = random_state_dict(N, 8)
    flat = pack_state_dict(sd)
    assert flat.dtype == torch.float32 and flat.numel() == packed_floats(N)
    assert same_bytes(flat.numpy(), host_pack(sd))  # the header's own pack
    back = unpack_to_state_dict(flat, N)
    assert list(back) == list(SailModule(N).state_dict()) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert torch.equal(pack_state_dict(back), flat)


def test_saved_file_loads_strict_and_gives_the_same_forward(tmp_path):
    N = 5
    sd = random_state_dict(N, 8)
    tr = SailTrainer(sd, device="cpu", lr=1e-3)
    assert tr.native is False and tr.flat.is_leaf and tr.flat.requires_grad and tr.flat.grad is not None
    robot, ob, target = plain_batch(N, 9, N, 45)
    tr.loss_and_grad(torch.from_numpy(robot), torch.from_numpy(ob), torch.from_numpy(target))
    tr.step()
    path = str(tmp_path / "sail_model.pth")
    tr.save(path)
    loaded = torch.load(path, map_location="cpu")
    m = SailModule(N)
    m.load_state_dict(loaded, strict=True)
    assert not all(torch.equal(loaded[k], sd[k]) for k in sd)  # the step moved the weights
    net = SailNet.load(path)
    a1, f1 = net.forward(torch.from_numpy(robot), torch.from_numpy(ob))
    a2, f2 = tr.net.forward(torch.from_numpy(robot), torch.from_numpy(ob))
    assert torch.equal(a1, a2) and torch.equal(f1, f2) and bool(torch.isfinite(a1).all())
    pad = pack_state_dict({k: torch.ones_like(v) for k, v in sd.items()}) == 0
    assert bool((tr.flat.detach()[pad] == 0).all()) and bool((tr.flat.grad[pad] == 0).all())


def test_autograd_path_equals_autograd_of_the_unpacked_module():
    N, E = 3, 11
    sd = random_state_dict(N, 8)
    robot, ob, target, n_rows, mask, live = masked_batch(N, E, N + 1, 46, poison=True)
    tr = SailTrainer(sd, device="cpu", native=False)
    loss, count = tr.loss_and_grad(torch.from_numpy(robot), torch.from_numpy(ob), torch.from_numpy(target), torch.from_numpy(n_rows),
                                   torch.from_numpy(mask))
    assert int(count) == int(live.sum()) and bool(torch.isfinite(tr.flat.grad).all())
    want, want_loss = torch_grad(unpack_to_state_dict(tr.flat, N), robot, ob, target, live, 1.0 / live.sum(), torch.float32)
    assert same_bytes(tr.flat.grad.numpy(), want.astype(np.float32)) and abs(float(loss) - want_loss) <= 1e-6 * want_loss
    with pytest.raises(NotImplementedError):
        SailTrainer(sd, device="cpu", native=True)


def test_bindings_match_the_header():
    """_capi.SYMBOLS lists exactly the header's functions, the ABI is still 1, and EbcSailGradArgs has the header's
    layout."""
    text = open(HEADER).read()
    names = re.findall(r"^(?:int|const char \*)\s*(ebc_\w+)\(", text, flags=re.M)
    assert set(names) == set(_capi.SYMBOLS) and len(names) == len(set(names))
    assert _abi.ABI_VERSION == 1 and re.search(r"#define EBC_ABI_VERSION 1\b", text)
    for name, n_args in (("ebc_sail_grad", 3), ("ebc_sail_packed_floats", 2), ("ebc_sail_get_packed", 3), ("ebc_sail_set_packed", 3)):
        m = re.search(r"int %s\(([^)]*)\);" % name, text)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int


def test_grad_args_layout(tmp_path):
    S = _abi.EbcSailGradArgs
    fields = [f for f, _ in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",sizeof(EbcSailGradArgs));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu",offsetof(EbcSailGradArgs,%s));' % f for f in fields)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", exe], check=True, timeout=120)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert sizes == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


def test_sixteen_samples_fitted_on_the_cpu():
    """200 Adam steps on a fixed set of 16 samples: the loss ends below its first step's."""
    N = 5
    robot, ob, target = plain_batch(N, 16, N, 47)
    demos = dict(robot=torch.from_numpy(robot), ob=torch.from_numpy(ob), target=torch.from_numpy(target),
                 n_rows=torch.full((16,), N, dtype=torch.int64))
    tr = SailTrainer(random_state_dict(N, 1), device="cpu", optimizer="adam", lr=1e-3)
    losses = fit(tr, demos, epochs=200, batch_size=16, generator=torch.Generator().manual_seed(5))
    print("first %.4g last %.4g" % (losses[0], losses[-1]))
    assert len(losses) == 200 and np.isfinite(losses).all() and losses[-1] < losses[0]
