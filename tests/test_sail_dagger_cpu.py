"""ebc_sail_dagger_k and the DAgger schedule, the part that needs no GPU: the entry in the header, the bindings and the built
library, the struct's layout; the Python surface; what is refused without a device; DaggerDataset, the beta schedule and
the mask on CPU tensors; the tools' options; and the rollout of every case of tests/sail_dagger_cases.py walked on the
oracle, so that what tests/test_sail_dagger_gpu.py compares is known to be finite, inside the scene and non-trivial."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ebcsim import _abi, _capi, sail_train
from sail_dagger_cases import AUTO, CASES, SAFETY, SCHEDULE, mask_of, oracle_walk, schedule_setup
from sail_rollout_cases import BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")
FIELDS = ["struct_size", "K", "human_policy", "flags", "expert_safety_space", "take_expert", "robot", "ob", "n_rows",
          "learner_action", "expert_action", "robot_action_out", "reward", "done", "info"]


# ------------------------------------------------------------------ 1. header, bindings, layout
def test_entry_in_header_bindings_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+ebc_sail_dagger_k\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 2 == len(_capi.SYMBOLS["ebc_sail_dagger_k"][1])
    assert _capi.SYMBOLS["ebc_sail_dagger_k"][0] is C.c_int
    assert "#define EBC_ABI_VERSION 1" in text and _abi.ABI_VERSION == 1
    assert hasattr(_capi.lib(), "ebc_sail_dagger_k")


def test_dagger_args_layout(tmp_path):
    S = _abi.EbcSailDaggerArgs
    assert [f for f, _ in S._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu",sizeof(EbcSailDaggerArgs),sizeof(EbcStepKArgs));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu",offsetof(EbcSailDaggerArgs,%s));' % f for f in FIELDS)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", exe], check=True, timeout=120)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert sizes == [C.sizeof(S), 112] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 104 and C.sizeof(_abi.EbcStepKArgs) == 112 and len(_abi.EbcStepKArgs._fields_) == 17


# ------------------------------------------------------------------ 2. the Python surface
def test_python_signatures():
    from ebcsim.batched import BatchedEnv
    p = inspect.signature(BatchedEnv.alloc_sail_dagger_outputs).parameters
    assert list(p) == ["self", "K", "optional"] and p["optional"].default == ("reward", "done", "info")
    p = inspect.signature(BatchedEnv.sail_dagger_k_device).parameters
    assert list(p) == ["self", "outputs", "K", "take_expert", "safety_space", "human_policy", "flags"]
    assert (p["take_expert"].default, p["safety_space"].default, p["human_policy"].default, p["flags"].default) == (
        None, 0.15, _abi.HUMAN_ORCA, 0)
    p = inspect.signature(sail_train.collect_dagger).parameters
    assert list(p) == ["env", "steps", "beta", "generator", "safety_space", "human_policy"]
    assert (p["generator"].default, p["safety_space"].default, p["human_policy"].default) == (None, 0.15, _abi.HUMAN_ORCA)
    p = inspect.signature(sail_train.dagger).parameters
    assert list(p)[:14] == ["env", "trainer", "rounds", "demo_steps", "dagger_steps", "epochs", "dagger_epochs", "batch_size", "beta0",
                            "beta_decay", "capacity", "generator", "safety_space", "on_round"]
    assert (p["beta0"].default, p["beta_decay"].default, p["safety_space"].default, p["on_round"].default) == (0.5, 0.5, 0.15, None)
    assert list(inspect.signature(sail_train.DaggerDataset.__init__).parameters) == ["self", "capacity"]
    assert callable(sail_train.DaggerDataset.append) and callable(sail_train.DaggerDataset.as_demos)


# ------------------------------------------------------------------ 3. refused without a device
def test_null_handle_and_null_args_are_refused():
    L = _capi.lib()
    a = _abi.EbcSailDaggerArgs()
    a.struct_size = C.sizeof(a)
    a.K = 1
    for args in (C.addressof(a), None):
        assert L.ebc_sail_dagger_k(None, args) == _abi.ERR_INVALID
        assert b"null handle" in L.ebc_last_error()


# ------------------------------------------------------------------ 4. the aggregate
def _samples(first, n, R=3):
    i = torch.arange(first, first + n, dtype=torch.float64)
    return dict(robot=i[:, None].repeat(1, 9), ob=i[:, None, None].repeat(1, R, 5), n_rows=torch.arange(first, first + n),
                target=i[:, None].repeat(1, 2), steps=n, episodes=1, executed=None)


def test_dagger_dataset_order_and_fifo():
    d = sail_train.DaggerDataset(10)
    assert len(d) == 0
    with pytest.raises(ValueError):
        d.as_demos()
    assert d.append(_samples(0, 4)) == 4 and d.append(_samples(4, 3)) == 7
    demos = d.as_demos()
    assert set(demos) == {"robot", "ob", "n_rows", "target", "steps"} and demos["steps"] == 7
    assert demos["n_rows"].tolist() == list(range(7)) and demos["robot"][:, 0].tolist() == list(range(7))
    assert d.append(_samples(7, 5)) == 10  # 12 arrived, the two oldest left
    demos = d.as_demos()
    for k, shape in (("robot", (10, 9)), ("ob", (10, 3, 5)), ("n_rows", (10,)), ("target", (10, 2))):
        assert tuple(demos[k].shape) == shape, k
        assert demos[k].reshape(10, -1)[:, 0].tolist() == list(range(2, 12)), k
        assert demos[k].untyped_storage().nbytes() == demos[k].numel() * demos[k].element_size(), k  # nothing kept beyond capacity
    assert d.append(_samples(100, 25)) == 10  # one append larger than the capacity: its newest 10
    assert d.as_demos()["n_rows"].tolist() == list(range(115, 125))
    with pytest.raises(ValueError):
        sail_train.DaggerDataset(0)


# ------------------------------------------------------------------ 5. the schedule's beta and the mask
def test_beta_schedule_and_mask():
    assert [sail_train.dagger_beta(i) for i in (1, 2, 3)] == [0.5, 0.25, 0.125]
    assert [sail_train.dagger_beta(i, 0.8, 0.5) for i in (1, 2)] == [0.8, 0.4] and sail_train.dagger_beta(4, 1.0, 1.0) == 1.0
    with pytest.raises(ValueError):
        sail_train.dagger_beta(0)
    gen = lambda: torch.Generator().manual_seed(3)  # noqa: E731
    a, b = sail_train.dagger_mask(20, 70, 0.5, "cpu", gen()), sail_train.dagger_mask(20, 70, 0.5, "cpu", gen())
    assert a.dtype == torch.bool and tuple(a.shape) == (20, 70) and torch.equal(a, b)
    assert torch.equal(a, torch.rand((20, 70), generator=gen()) < 0.5)
    assert 0.4 < float(a.float().mean()) < 0.6
    assert sail_train.dagger_mask(20, 70, 0.0, "cpu", gen()) is None  # the entry's NULL
    assert bool(sail_train.dagger_mask(4, 4, 1.0, "cpu", gen()).all())


# ------------------------------------------------------------------ 6. the tools
def test_tools_list_the_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_sail.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for opt in ("--dagger-rounds", "--dagger-steps", "--dagger-epochs", "--beta0", "--beta-decay", "--capacity"):
        assert opt in r.stdout, opt
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sail_dagger_bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0
    for opt in ("--envs", "--steps", "--blocks"):
        assert opt in r.stdout, opt


# ------------------------------------------------------------------ 7. the cases, walked on the oracle
def test_cases_cover_what_the_issue_lists():
    assert len({c[0] for c in CASES}) == len(CASES) == 8
    assert [c[1] for c in CASES] == [5, 5, 2, 10, 11, 17, 32, 5]
    assert [(c[2], c[3]) for c in CASES][:4] == [(5, 0), (3, 2), (2, 0), (8, 2)]
    assert [(c[5], c[6]) for c in CASES] == [(70, 20), (3, 20), (70, 6), (70, 6), (7, 3), (4, 3), (3, 3), (1, 1)]
    assert CASES[0][7:] == (AUTO, 140, False, "random") and CASES[1][4] == 13 and CASES[1][7:] == (AUTO, 0, True, "random")
    assert CASES[2][10] is None and CASES[3][10] == "ones"
    assert all(c[1] == c[2] + c[3] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_oracle_walk_is_finite_inside_and_not_trivial(case):
    tag, A, humans, static, T, E, K, flags, pool, sim, kind = case
    out, state, where = oracle_walk(case)
    mask = mask_of(case)
    for name in ("learner_action", "expert_action", "robot_action_out"):
        assert out[name].shape == (K, E, 2) and np.isfinite(out[name]).all(), (tag, name)
    assert where.shape == (K + 1, E, 2) and (np.abs(where) < BOUND).all(), (tag, float(np.abs(where).max()))
    assert (out["n_rows"] == A).all(), tag
    assert out["ob"].shape == (K, E, A, 5) and out["robot"].shape == (K, E, 9)
    if flags and K == 20:
        assert int(out["done"].sum()) > E, tag  # restarts inside the window
    if kind == "random":
        assert mask.any() and not mask.all(), tag
    # the mask decides something: the two actions differ where it matters
    differ = (out["learner_action"] != out["expert_action"]).any(axis=2)
    assert differ.any(), tag
    taken = out["robot_action_out"]
    if mask is None:
        assert (taken == out["learner_action"]).all()
    else:
        m = mask.astype(bool)
        assert (taken[m] == out["expert_action"][m]).all() and (taken[~m] == out["learner_action"][~m]).all()


def test_schedule_scenes_give_demonstrations():
    """The batch of the schedule test: with the demonstrator driving (persistent simulator, as collect_sail_demos runs it)
    episodes end in ReachGoal inside the window, so round 0 has samples to fit."""
    from oracle import oracle
    params, batch, _ = schedule_setup()
    o = oracle.OracleEnv(params, batch.n, batch.N, batch.S)
    o.reset(batch)
    o.robot_orca_sim(True)
    reached = 0
    for k in range(SCHEDULE["demo_steps"]):
        step = o.step(robot_action=o.robot_orca(SAFETY), human_policy=_abi.HUMAN_ORCA, flags=AUTO)
        reached += int(((step["done"] != 0) & (step["info"] == _abi.INFO_REACH_GOAL)).sum())
    assert reached >= 8, reached
