"""The layer form of the SARL gradient without a device: the WIDE host build of the rule header
(tests/native/sarl_grad_layers_host.cc: the serial loops' buffers 640 floats a row) gives the narrow build's bytes, the new
limits (grad_dims_refused_layers: 640 is taken, 641 is not; the chunk form's stay at 256), the rule's accuracy at the x2 and
x4 widths against float64 autograd (profiles/sarl_grad_layers_accuracy.txt), the sanitizer build of the stand-alone
program, and SarlFormTrainer(grad_form=...)'s argument checks."""
import os
import subprocess

import numpy as np
import pytest

import sarl_grad_cases as base
import sarl_grad_layers_cases as wide
from sarl_grad_cases import NETS, REFERENCE_WIDTHS, ROOT, TOL_FACTOR, same_bytes


def _same(got, want, tag):
    assert same_bytes(got[0], want[0]), (tag, "grad")
    assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes() and got[2] == want[2], (tag, "loss_sum, count")
    assert same_bytes(got[3], want[3]) and same_bytes(got[4], want[4]), (tag, "value, attention")


def test_constants_of_the_header():
    assert wide.constant("max_width") == 640 and wide.constant("max_rows") == 128 and wide.constant("stride") == 640
    assert wide.constant("run_slots") % (wide.constant("chunk") * wide.constant("max_rows")) == 0  # a run of R = 128 is whole chunks
    assert wide.constant("chunk") == base.chunk()
    from ebcsim import sarl_train
    assert sarl_train.MAX_WIDTH_LAYERS == 640 and sarl_train.MAX_ROWS_LAYERS == 128 and sarl_train.MAX_WIDTH == 256


@pytest.mark.parametrize("ni", [0, 1, 2, 3])
def test_the_wide_build_gives_the_narrow_builds_bytes(ni):
    """The stride of the serial loops' buffers moves no byte: NETS[0 .. 3] at B in 1, 5, 9 and R in 1, 5, on plain and edge
    batches; the packed image too."""
    net = NETS[ni]
    sd = base.random_state_dict(net)
    P = base.host_pack(sd)
    assert same_bytes(wide.host_pack(sd), P) and wide.host_floats(net) == base.host_floats(net)
    for B in (1, 5, 9):
        for R in (1, 5):
            rows, target = base.plain_batch(net, B, R)
            _same(wide.host_grad(P, net, rows, target, None, None, 2.0 / B), base.host_grad(P, net, rows, target, None, None, 2.0 / B), ("plain", B, R))
            rows, target, nv, mask, kinds = base.edge_batch(net, B, R)
            _same(wide.host_grad(P, net, rows, target, nv, mask, 2.0 / B), base.host_grad(P, net, rows, target, nv, mask, 2.0 / B), ("edge", B, R, kinds))


def test_every_refusal_code_of_the_layer_forms_limits():
    ref = REFERENCE_WIDTHS

    def with_(i, v):
        out = list(ref)
        out[i] = v
        return out
    assert wide.refused(ref) == 0 and wide.refused(wide.X2_WIDTHS) == 0 and wide.refused(wide.X4_WIDTHS) == 0
    assert wide.refused(with_(0, 0)) == 1 and wide.refused(with_(0, 65)) == 1 and wide.refused(with_(0, 64)) == 0
    for l in range(11):
        last = l in (6, 10)
        assert wide.refused(with_(l + 1, 0)) == l + 2 and wide.refused(with_(l + 1, 641)) == l + 2
        assert wide.refused(with_(l + 1, 640)) == (l + 2 if last else 0) and wide.refused(with_(l + 1, 2)) == (l + 2 if last else 0)
        # the chunk form's limits are where they were
        assert wide.refused(with_(l + 1, 257), chunk_form=True) == l + 2
        assert wide.refused(with_(l + 1, 256), chunk_form=True) == (l + 2 if last else 0)
    assert wide.refused(ref, self_dim=-1) == 13 and wide.refused(ref, self_dim=14) == 13 and wide.refused(ref, self_dim=13) == 0
    assert wide.refused(ref, om_width=-1) == 14 and wide.refused(ref, om_width=193) == 14 and wide.refused(ref, om_width=192) == 0
    assert wide.refused(with_(0, 33), om_width=192) == 15 and wide.refused(with_(0, 32), om_width=192) == 0
    assert wide.refused(with_(0, 64), om_width=160) == 0 and wide.refused(with_(0, 64), om_width=161) == 15
    # the order of the codes is grad_dims_refused_wide's: the row, the layers ascending, the self state, the map
    assert wide.refused(with_(0, 65), self_dim=99, om_width=999) == 1 and wide.refused(with_(3, 641), self_dim=99, om_width=999) == 4
    assert wide.refused(ref, self_dim=99, om_width=999) == 13
    assert wide.refused(with_(3, 641), self_dim=99, om_width=999, chunk_form=True) == 4 and wide.refused(ref, self_dim=99, om_width=999, chunk_form=True) == 13


@pytest.mark.parametrize("name,B,R", [(n, B, R) for n, _, B, R in wide.ACCURACY_CASES])
def test_the_rule_at_the_wide_widths_against_float64_autograd(name, B, R):
    """Per layer and for the loss, the rule's error against float64 autograd stays within TOL_FACTOR times torch's own
    float32 error (tests/sarl_grad_cases.py: the bar and the seeds)."""
    net = wide.X2_NET if name == "x2" else wide.X4_NET
    layers, (loss_err, loss32), seed = wide.accuracy_row(net, B, R)
    for key, err, err32 in layers:
        print("%s B %d R %d seed %d %-12s rule %.3e torch32 %.3e ratio %.2f" % (name, B, R, seed, key, err, err32, err / err32))
        assert err <= TOL_FACTOR * err32, (key, err, err32)
    print("%s B %d R %d loss rule %.3e torch32 %.3e" % (name, B, R, loss_err, loss32))
    assert loss_err <= TOL_FACTOR * loss32


def test_the_accuracy_profile_is_the_table_of_these_cases():
    """profiles/sarl_grad_layers_accuracy.txt is what tests/sarl_grad_layers_cases.py writes: the same cases and layers,
    every ratio within the bar (the figures themselves depend on the machine's torch build in the last digits)."""
    lines = open(os.path.join(ROOT, "profiles", "sarl_grad_layers_accuracy.txt")).read().splitlines()
    body = [l.split() for l in lines if l[:2] in ("x2", "x4") and ":" not in l.split()[0]]
    cases = {(p[0], int(p[1]), int(p[2])) for p in body}
    assert cases == {(n, B, R) for n, _, B, R in wide.ACCURACY_CASES}
    assert len(body) == 12 * len(wide.ACCURACY_CASES) and all(float(p[-1]) <= TOL_FACTOR for p in body)


def test_the_sanitizer_build_of_the_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on the stand-alone program (a process of its own: nothing of it is loaded here): one x2 batch and one
    edge batch of the narrow network run clean and give the shared library's bytes."""
    sd2, sd1 = base.random_state_dict(wide.X2_NET), base.random_state_dict(NETS[1])
    rows2, target2 = base.plain_batch(wide.X2_NET, 5, 3)
    rows1, target1, nv, mask, _ = base.edge_batch(NETS[1], 9, 5)
    batches = [(wide.X2_NET, wide.host_pack(sd2), rows2, target2, None, None, 0.4), (NETS[1], wide.host_pack(sd1), rows1, target1, nv, mask, 2.0 / 9)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    wide.write_batches(src, batches)
    run = subprocess.run([wide.host_program(sanitize=True), src, dst], check=True, capture_output=True, text=True, timeout=300)
    assert "sarl_grad_layers_host: 2 batches" in run.stdout and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    for got, (net, P, rows, target, n_valid, m, scale) in zip(base.read_results(dst, batches), batches):
        _same(got, wide.host_grad(P, net, rows, target, n_valid, m, scale), ("program", net[0][1]))


def test_trainer_argument_checks_without_a_device():
    from ebcsim.sarl_train import SarlFormTrainer, SarlTrainer
    import inspect
    # SarlTrainer is the object it was: the choice of the form is SarlFormTrainer's
    assert "grad_form" not in inspect.signature(SarlTrainer.__init__).parameters and issubclass(SarlFormTrainer, SarlTrainer)
    sd = base.random_state_dict(NETS[1])
    for form in (None, "chunk", "layers", "auto"):
        tr = SarlFormTrainer(sd, device="cpu", grad_form=form)  # native=False on the CPU: grad_form is ignored
        assert tr.grad_form == form and not tr.native and tr.net is None
    with pytest.raises(ValueError, match="grad_form"):
        SarlFormTrainer(sd, device="cpu", grad_form="rows")
    with pytest.raises(ValueError, match="two answers"):
        SarlFormTrainer(sd, device="cpu", grad_form="auto", states_per_pass=2)
    with pytest.raises(ValueError, match="two answers"):
        SarlFormTrainer(sd, device="cpu", grad_form="auto", states_per_pass="auto")
    with pytest.raises(ValueError, match="no passes"):
        SarlFormTrainer(sd, device="cpu", grad_form="layers", states_per_pass=1)
    assert SarlFormTrainer(sd, device="cpu", grad_form="chunk", states_per_pass=2).states_per_pass == 2
    with pytest.raises(NotImplementedError, match="HIP device"):
        SarlFormTrainer(sd, device="cpu", grad_form="layers", native=True)
    # the wide network trains on the CPU through autograd whatever the form
    tr = SarlFormTrainer(base.random_state_dict(wide.X2_NET), device="cpu", grad_form="auto")
    rows, target = base.plain_batch(wide.X2_NET, 3, 2)
    import torch
    loss, count = tr.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target), grad_scale=2.0 / 3)
    assert int(count) == 3 and np.isfinite(float(loss)) and tr.form_of(2) == "layers"
