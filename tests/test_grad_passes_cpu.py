"""What the pass form of the two gradient kernels (states_per_pass) has on the host: the C ABI's new entries and the renamed
struct field against the header, the choice "auto" makes, the trainers' checks of the setting, and the accuracy yardstick of
the unchanged rule headers at the row counts the passes open up (16, 30 and 33 rows per state).  The kernels themselves:
tests/test_grad_passes_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lstm_grad_cases as lg
import sarl_grad_cases as sg
from cadrl_cases import TOL_FACTOR
from ebcsim import _abi, _capi
from ebcsim.lstm_train import LstmTrainer
from ebcsim.sarl_train import PASS_SIZES, PassChoice, SarlTrainer, checked_states_per_pass, pick_states_per_pass

HEADER = os.path.join(sg.ROOT, "include", "ebcsim.h")
NEW_ENTRIES = (("ebc_sarl_net_grad_max_rows_at", 3), ("ebc_lstm_net_grad_max_rows_at", 3))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_bindings_match_the_header():
    text = open(HEADER).read()
    names = re.findall(r"^(?:int|const char \*)\s*(ebc_\w+)\(", text, flags=re.M)
    assert set(names) == set(_capi.SYMBOLS) and len(names) == len(set(names))
    for name, n_args in NEW_ENTRIES:
        m = re.search(r"int %s\(([^)]*)\);" % name, text)
        assert m and len(m.group(1).split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        assert _capi.SYMBOLS[name][0] is C.c_int and _capi.SYMBOLS[name][1][1] is C.c_int
        assert "int states_per_pass" in m.group(1)


@pytest.mark.parametrize("name", ["EbcSarlGradArgs", "EbcLstmGradArgs"])
def test_struct_layouts_match_the_header(name, tmp_path):
    S = getattr(_abi, name)
    fields = [f for f, _ in S._fields_]
    assert "states_per_pass" in fields and "reserved" not in fields
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",sizeof(%s));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, name, "\n".join('printf(" %%zu",offsetof(%s,%s));' % (name, f) for f in fields)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", exe], check=True, timeout=120)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert sizes == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert S.states_per_pass.offset == 20 and S.states_per_pass.size == 4  # where `reserved` was: a zeroed struct is today's call


# ---------------------------------------------------------------------------------------------- "auto"
SARL_LIMITS = (15, {4: 15, 2: 32, 1: 64})       # the reference widths
LSTM_LIMITS = (12, {4: 12, 2: 25, 1: 52})       # with mlp1
CHOICES = [(SARL_LIMITS, 1, 0), (SARL_LIMITS, 5, 0), (SARL_LIMITS, 10, 0), (SARL_LIMITS, 15, 0), (SARL_LIMITS, 16, 2), (SARL_LIMITS, 30, 2),
           (SARL_LIMITS, 32, 2), (SARL_LIMITS, 33, 1), (SARL_LIMITS, 64, 1), (SARL_LIMITS, 65, 1),
           (LSTM_LIMITS, 12, 0), (LSTM_LIMITS, 13, 2), (LSTM_LIMITS, 25, 2), (LSTM_LIMITS, 26, 1), (LSTM_LIMITS, 30, 1), (LSTM_LIMITS, 52, 1),
           (LSTM_LIMITS, 53, 1),
           ((3, {4: 2, 2: 7, 1: 15}), 3, 0),    # the whole chunk's limit is asked on its own and wins where it holds R
           ((0, {4: 0, 2: 1, 1: 2}), 1, 2)]


@pytest.mark.parametrize("limits,R,want", CHOICES)
def test_auto_picks_the_largest_pass_that_holds_the_rows(limits, R, want):
    """0 (the default call) where the whole chunk fits, else the largest S in 4, 2, 1 whose limit holds R; past every limit 1,
    which the kernel then refuses by name."""
    assert PASS_SIZES == (4, 2, 1)
    assert pick_states_per_pass(R, limits[0], limits[1]) == want


class FakeNet(object):
    def __init__(self, limits):
        self.whole, self.at, self.asked = limits[0], limits[1], []

    def grad_max_rows(self, states_per_pass=0):
        self.asked.append(states_per_pass)
        return self.whole if states_per_pass == 0 else self.at[states_per_pass]


def test_a_trainers_choice_and_limit():
    net = FakeNet(SARL_LIMITS)
    none, auto, two = PassChoice(net, None), PassChoice(net, "auto"), PassChoice(net, 2)
    assert sorted(net.asked) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 4, 4, 4]  # asked once per trainer, not per call
    assert [none.of(R) for R in (5, 16, 99)] == [0, 0, 0] and none.max_rows() == 15
    assert [auto.of(R) for R in (5, 15, 16, 33, 99)] == [0, 0, 2, 1, 1] and auto.max_rows() == 64
    assert [two.of(R) for R in (5, 16, 99)] == [2, 2, 2] and two.max_rows() == 32


@pytest.mark.parametrize("bad", [0, 3, 5, -1, 8, "2", "AUTO", 2.0, True])
def test_other_settings_raise(bad):
    sd = sg.random_state_dict(sg.NARROW_NET)
    with pytest.raises(ValueError, match="states_per_pass"):
        checked_states_per_pass(bad, "test")
    with pytest.raises(ValueError, match="SarlTrainer: states_per_pass"):
        SarlTrainer(sd, device="cpu", native=False, states_per_pass=bad)
    with pytest.raises(ValueError, match="LstmTrainer: states_per_pass"):
        LstmTrainer(lg.random_state_dict(lg.NARROW_NET2), device="cpu", native=False, states_per_pass=bad)


@pytest.mark.parametrize("setting", [None, "auto", 1, 2, 4])
def test_the_autograd_trainers_ignore_the_setting(setting):
    """native=False: the setting is kept and changes nothing, 30 rows per state included."""
    assert checked_states_per_pass(setting, "test") == setting
    for Trainer, cases, net in ((SarlTrainer, sg, sg.NARROW_NET), (LstmTrainer, lg, lg.NARROW_NET2)):
        sd = cases.random_state_dict(net)
        rows, target = cases.plain_batch(net, 5, 30, seed=77)
        a, b = Trainer(sd, device="cpu", native=False, states_per_pass=setting), Trainer(sd, device="cpu", native=False)
        assert a.states_per_pass == setting and a.net is None and not a.native
        la, ca = a.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target))
        lb, cb = b.loss_and_grad(torch.from_numpy(rows), torch.from_numpy(target))
        assert float(la) == float(lb) and int(ca) == int(cb) == 5 and torch.equal(a.flat.grad, b.flat.grad)
    with pytest.raises(NotImplementedError, match="needs a HIP device"):
        SarlTrainer(sg.random_state_dict(sg.NARROW_NET), device="cpu", native=True, states_per_pass=setting)


# ---------------------------------------------------------------------------------------------- the yardstick at the new row counts
@pytest.mark.parametrize("B,R", [(100, 16), (100, 30), (9, 30)])
def test_the_sarl_rule_against_float64_autograd_at_the_new_row_counts(B, R):
    """tests/test_sarl_train_cpu.py's test_host_build_against_float64_autograd at the reference widths with 16 and 30 rows
    per state: a chain of 4 R terms stays within TOL_FACTOR times torch's own float32 error, per layer and for the loss."""
    layers, (loss_rule, loss_t32), (min_score, min_den), seed = sg.accuracy_row(0, B, R)
    for name, err_rule, err_t32 in layers + [("loss_sum", loss_rule, loss_t32)]:
        print("B %3d R %2d seed %d %-14s rule %.3e torch32 %.3e ratio %.2f" % (B, R, seed, name, err_rule, err_t32, err_rule / err_t32))
    assert min_score > 0 and min_den > 0, (min_score, min_den)
    for name, err_rule, err_t32 in layers + [("loss_sum", loss_rule, loss_t32)]:
        assert err_t32 >= sg.YARDSTICK_FLOOR and err_rule <= TOL_FACTOR * err_t32, (name, err_rule, err_t32)


@pytest.mark.parametrize("scale", lg.SCALES)
@pytest.mark.parametrize("B,R", [(100, 30), (9, 33)])
@pytest.mark.parametrize("ni", [0, 1], ids=["mlp1", "plain"])
def test_the_lstm_rule_against_float64_autograd_at_the_new_row_counts(ni, B, R, scale):
    """tests/test_lstm_train_cpu.py's test_the_rule_against_float64_autograd at the reference widths with 30 and 33 steps,
    both networks, gate scales 1 and 4; the floor as there."""
    tensors, (lr, lt), seed = lg.accuracy_row(("seeded", ni, B, R, scale))
    for key, er, et in tensors + [("loss_sum", lr, lt)]:
        print("seed %d %-22s rule %.3e torch32 %.3e ratio %.2f" % (seed, key, er, et, er / et if et else float("inf")))
    for key, er, et in tensors + [("loss_sum", lr, lt)]:
        assert et >= lg.YARDSTICK_FLOOR, (key, et)
        assert er <= TOL_FACTOR * max(et, lg.YARDSTICK_FLOOR), (key, er, et)
    assert np.isfinite(lr)
