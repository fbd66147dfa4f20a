"""The wide value-network blocks without a GPU: which entry makes each block of a network (ebcsim.sarl.plan_blocks, from
shapes alone), the paths select_path gives a network with wide blocks, the C ABI, and the `wide` keyword on its way from
the tools through run_sarl_training and SarlModule.as_value_net to SarlValueNet."""
import importlib.util
import os
import re
import sys

import pytest
import torch

import value_net_cases as vc
import vn_wide_cases as wc
from ebcsim.mlp2 import Mlp2Block
from ebcsim.sarl import block_kind, plan_blocks, plan_facts, select_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eb-cadrl_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


# ---- block specs ------------------------------------------------------------------------------------------------------------
def test_block_kind_at_both_limits():
    assert block_kind(224, 320, 224, False) == block_kind(224, 320, 224, True) == "narrow"
    for shape in ((225, 320, 224), (224, 321, 224), (224, 320, 225)):
        assert block_kind(*shape, False) is None and block_kind(*shape, True) == "wide", shape
    assert block_kind(640, 640, 640, True) == "wide"
    for shape in ((641, 640, 640), (640, 641, 640), (640, 640, 641)):
        assert block_kind(*shape, True) is None, shape
    assert Mlp2Block.WIDE_MAX == wc.LIMIT and Mlp2Block.WIDE_ROWS_PER_WORKGROUP == wc.ROWS_PER_WORKGROUP


@pytest.mark.parametrize("name", sorted(wc.PLANS))
def test_plan_of_the_networks(name):
    """x2 is narrow blocks either way; x3 and x4 have no blocks without `wide` and wide ones with it; the hidden-512
    network gets ONE wide block (mlp1) beside today's narrow ones; beyond 640 there are no blocks."""
    dims, T, narrow, wide = wc.PLANS[name]
    shapes = wc.stack_shapes(dims, T)
    norm = lambda p: None if p is None else (list(p[0]), p[1])  # noqa: E731
    assert norm(plan_blocks(*shapes, False)) == norm(narrow), name
    assert norm(plan_blocks(*shapes, True)) == norm(wide), name


def test_plan_refuses_other_layer_counts_and_scores():
    m1, m2, att, m3 = wc.stack_shapes(wc.X4, 17)
    assert plan_blocks(m1 + [(10, 400)], m2, att, m3, True) is None
    assert plan_blocks(m1, m2, att[:2] + [(2, 400)], m3, True) is None
    kinds, gterm = plan_blocks(m1, m2, att, m3[:2], True)  # mlp3 of two layers: torch for it
    assert len(kinds) == 3 and gterm == "wide"


def test_the_kernel_constants_are_the_cases():
    h = _read(CSRC, "ebc_vn_wide.h")
    assert re.search(r"#define EBC_VNW_MAX %d\b" % wc.LIMIT, h)
    assert re.search(r"#define EBC_VNW_NW %d\b" % (wc.ROWS_PER_WORKGROUP // 32), h) and "#define EBC_VNW_ROWS (32 * EBC_VNW_NW)" in h
    # the narrow entries keep their limits and their refusal
    assert "K0 > 224 || O > 224 || H > 320" in _read(CSRC, "ebcsim_value_net.hip")


# ---- path table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["x3", "x4", "hidden512"])
def test_a_network_with_wide_blocks_takes_blocks_and_exact_native(name):
    """A wide mlp1 or mlp2 has no tile epilogue and no fragment twins: the coarse forward is "blocks" at every pair size,
    the exact one the library's float32 form; autograd and the CPU stay torch's.  select_path has no branch for it."""
    dims, T, _, _ = wc.PLANS[name]
    shapes = wc.stack_shapes(dims, T)
    facts = plan_facts(plan_blocks(*shapes, True), shapes[0], shapes[1])
    assert facts.n_blocks == 5 and facts.gterm and not facts.frag and not facts.mlp1_epilogue
    for R in vc.NETWORK_ROWS:
        for frag_handoff in (False, True):
            assert select_path(facts, "cuda", frag_handoff, True, R, T, False, False, False) == "blocks"
            assert select_path(facts, "cuda", frag_handoff, True, R, T, False, True, False) == "blocks"
            assert select_path(facts, "cuda", frag_handoff, True, R, T, True, False, False) == "exact_native"
            assert select_path(facts, "cuda", frag_handoff, False, R, T, True, False, False) == "torch"
            for exact in (False, True):
                assert select_path(facts, "cuda", frag_handoff, True, R, T, exact, False, True) == "torch"
                assert select_path(facts, "cpu", frag_handoff, True, R, T, exact, False, False) == "torch"
    # without the keyword: no blocks, torch everywhere (what the existing tests pin)
    none = plan_facts(plan_blocks(*shapes, False), shapes[0], shapes[1])
    assert none.n_blocks == 0
    assert {select_path(none, "cuda", True, True, R, T, e, False, False) for R in vc.NETWORK_ROWS for e in (False, True)} == {"torch"}


def test_the_narrow_network_keeps_its_facts_with_the_keyword():
    dims, T, _, _ = wc.PLANS["x2"]
    shapes = wc.stack_shapes(dims, T)
    a, b = (plan_facts(plan_blocks(*shapes, w), shapes[0], shapes[1]) for w in (False, True))
    assert a == b and a.frag and a.mlp1_epilogue and a.mlp2_epilogue and a.n_blocks == 5


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_in_the_header_and_the_bindings():
    from ebcsim import _capi
    header = _read(ROOT, "include", "ebcsim.h")
    assert re.search(r"\bint ebc_mlp2_create_wide\(int device_id, int K0, int H, int O,", header)
    assert "ebc_mlp2_create_wide" in _read(ROOT, "eb-cadrl_amd", "ebcsim", "_capi.py")
    lib = _capi.lib()
    assert lib.ebc_mlp2_create_wide.argtypes == lib.ebc_mlp2_create_ex.argtypes


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def test_as_value_net_passes_wide_through(monkeypatch):
    from ebcsim import train
    seen = []

    def from_stacks(*a, **kw):
        seen.append(kw)
        return "net"
    monkeypatch.setattr(train.SarlValueNet, "from_stacks", staticmethod(from_stacks))
    m = train.SarlModule(13, [32, 16], [16, 8], [16, 8, 8, 1], [16, 16, 1])
    assert m.as_value_net() == "net" and m.as_value_net(native=True) == "net" and m.as_value_net(True, wide=True) == "net"
    assert seen == [{}, {}, {"wide": True}]


def test_sarl_value_net_keeps_the_keyword_on_every_constructor():
    from ebcsim.sarl import SarlValueNet
    sd = vc.network_state_dict(vc.SMALL, 13, seed=1)
    assert SarlValueNet(sd).wide is False and SarlValueNet(sd, wide=True).wide is True
    a = SarlValueNet(sd)
    for w in (False, True):
        assert SarlValueNet.from_stacks(a.mlp1, a.mlp2, a.attention, a.mlp3, True, 6, "cpu", wide=w).wide is w
    # a CPU network has no blocks whatever the keyword says
    assert SarlValueNet(sd, wide=True)._block_specs() is None


@pytest.mark.parametrize("wide", [False, True])
def test_run_sarl_training_passes_wide_decide_through(monkeypatch, wide):
    from ebcsim import grad_train, sarl_train
    seen = []

    class Net(object):
        def __init__(self, sd, **kw):
            seen.append(kw)

    def schedule(env, trainer, gamma, width, new_net, *rest):
        new_net()
        new_net()  # the deciding and the target network
        return {}
    monkeypatch.setattr(sarl_train, "SarlValueNet", Net)
    monkeypatch.setattr(grad_train, "run_value_training", schedule)

    class Trainer(object):
        device, widths, om_width, native, with_global_state, self_state_dim = torch.device("cuda", 0), [13], 0, False, True, 6

        def state_dict(self):
            return {}

    class Env(object):
        T, R = 13, 5
    if wide:
        sarl_train.run_sarl_training_ex(Env(), Trainer(), None, 0.9, wide_decide=True)
    else:
        sarl_train.run_sarl_training(Env(), Trainer(), None, 0.9)
    assert len(seen) == 2 and all(("wide" in k) == wide for k in seen) and all(k.get("wide", False) is wide for k in seen)


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name[:-3], os.path.join(ROOT, "tools", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _FakeEnv(object):
    T, R, E = 13, 5, 2

    def __init__(self, *a, **kw):
        pass

    def __getattr__(self, name):  # generate_reset, generate_pool, synchronize, use_torch_stream, close
        return lambda *a, **kw: None


def _record_load(monkeypatch):
    """SarlValueNet.load records its keywords and ends the tool there; the env is a stand-in (no device)."""
    from ebcsim import batched, sarl
    seen = []

    def load(path, device="cpu", **kw):
        seen.append(kw)
        raise _Stop()
    monkeypatch.setattr(sarl.SarlValueNet, "load", staticmethod(load))
    monkeypatch.setattr(batched, "BatchedEnv", _FakeEnv)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    return seen


@pytest.mark.parametrize("wide", [False, True])
def test_evaluate_tool_passes_wide_through(monkeypatch, wide):
    seen = _record_load(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["evaluate.py", "--policy", "sarl", "--weights", "w.pth", "--device-scenes", "--cases", "2",
                                      "--env-config", os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"),
                                      "--policy-config", os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_x3.config")]
                        + (["--wide-decide"] if wide else []))
    with pytest.raises(_Stop):
        _tool("evaluate.py").main()
    assert seen == ([{"wide": True}] if wide else [{}])


@pytest.mark.parametrize("wide", [False, True])
def test_train_tool_passes_wide_through(monkeypatch, wide, tmp_path):
    """tools/train_sarl.py --wide-decide: wide_decide=True to run_sarl_training_ex and wide=True to the network its
    evaluations load; without the flag neither keyword is passed."""
    from ebcsim import sarl_train
    seen = _record_load(monkeypatch)
    calls = []

    def schedule(name):
        def run(env, trainer, space, gamma, after_il=None, **kw):
            calls.append((name, kw))
            after_il({"il_stored": 0, "il_episodes": 0})  # the first evaluation: loads the saved network
        return run

    class Trainer(object):
        def __init__(self, *a, **kw):
            pass

    class Gen(object):
        def __init__(self, *a, **kw):
            pass

        def manual_seed(self, seed):
            return self
    monkeypatch.setattr(sarl_train, "run_sarl_training", schedule("plain"))
    monkeypatch.setattr(sarl_train, "run_sarl_training_ex", schedule("ex"))
    monkeypatch.setattr(sarl_train, "SarlFormTrainer", Trainer)
    monkeypatch.setattr(torch, "Generator", Gen)
    monkeypatch.setattr(sys, "argv", ["train_sarl.py", "--device-scenes", "--envs", "2", "--grad-form", "auto",
                                      "--env-config", os.path.join(ROOT, "eb-cadrl_amd", "configs", "sarl_a5.config"),
                                      "--policy-config", os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_x3.config"),
                                      "--out", str(tmp_path / "m.pth")] + (["--wide-decide"] if wide else []))
    with pytest.raises(_Stop):
        _tool("train_sarl.py").main()
    assert len(calls) == 1 and calls[0][0] == ("ex" if wide else "plain")
    assert ("wide_decide" in calls[0][1]) == wide and calls[0][1].get("wide_decide", False) is wide
    assert seen == ([{"with_global_state": True, "wide": True}] if wide else [{"with_global_state": True}])


def test_the_x3_config_holds_the_x3_widths():
    import configparser
    pol = configparser.RawConfigParser()
    pol.read(os.path.join(ROOT, "eb-cadrl_amd", "configs", "policy_x3.config"))
    got = {k: tuple(int(x) for x in pol.get("sarl", k + "_dims").split(",")) for k in ("mlp1", "mlp2", "attention", "mlp3")}
    assert got == wc.X3
