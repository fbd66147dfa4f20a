"""ebc_step_k with EBC_ROBOT_SAIL, the part that needs no GPU: the enum and the attach entry in the header, the bindings
and the built library; the Python surface; the windowed evaluation path's option; and the reference rollout of
tests/test_sail_rollout_gpu.py (the oracle's step with the g++ host build deciding) walked over every test configuration:
every action finite, every robot inside the scene's bounds at every step, every env with adult_num rows at every step."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ebcsim import _abi, _capi
from sail_rollout_cases import ARRIVED_ENV, BITWISE, BOUND, reference_rollouts, oracle_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")


def test_enum_and_entry_in_header_and_bindings():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bEBC_ROBOT_SAIL\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 3 == _abi.ROBOT_SAIL
    assert (_abi.ROBOT_EXTERNAL, _abi.ROBOT_LINEAR, _abi.ROBOT_ORCA) == (0, 1, 2)
    m = re.search(r"\bint\s+ebc_robot_sail\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 2 == len(_capi.SYMBOLS["ebc_robot_sail"][1])
    assert _capi.SYMBOLS["ebc_robot_sail"][0] is C.c_int
    assert "#define EBC_ABI_VERSION 1" in text and _abi.ABI_VERSION == 1


def test_step_k_args_did_not_grow(tmp_path):
    """The attach call carries the network: EbcStepKArgs has the layout it had (17 fields, 112 bytes)."""
    S = _abi.EbcStepKArgs
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(EbcStepKArgs));return 0;}\n' % HEADER)
    subprocess.check_call(["gcc", "-o", str(tmp_path / "size"), str(src)])
    assert int(subprocess.check_output([str(tmp_path / "size")])) == C.sizeof(S) == 112 and len(S._fields_) == 17


def test_library_exports_the_entry():
    L = _capi.lib()  # raises if the product library lacks a symbol the bindings list
    assert hasattr(L, "ebc_robot_sail") and hasattr(L, "ebc_step_k") and hasattr(L, "ebc_sail_create")


def test_python_surface():
    from ebcsim.batched import BatchedEnv
    from ebcsim.sail import DeviceSailPolicy
    from ebcsim.train import evaluate_windows
    assert list(inspect.signature(BatchedEnv.attach_sail).parameters) == ["self", "net"]
    sig = inspect.signature(DeviceSailPolicy.rollout)
    assert list(sig.parameters) == ["self", "env", "K", "outputs", "flags", "human_policy"]
    assert sig.parameters["flags"].default == 0 and sig.parameters["human_policy"].default == _abi.HUMAN_ORCA
    for fn in (BatchedEnv.step_k, BatchedEnv.step_k_device):
        assert "robot_policy" in inspect.signature(fn).parameters
    assert list(inspect.signature(evaluate_windows).parameters) == ["env", "rollout", "gamma", "steps_per_call", "max_steps"]


def test_evaluate_takes_steps_per_call():
    path = os.path.join(ROOT, "tools", "evaluate.py")
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--steps-per-call" in r.stdout and "--one-launch" in r.stdout
    r = subprocess.run([sys.executable, path, "--policy", "orca", "--steps-per-call", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--policy sail" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sail_rollout_bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "one-launch" in r.stdout


def test_cases_cover_what_the_issue_lists():
    col = lambda i: {c[i] for c in BITWISE}  # noqa: E731
    assert col(1) >= {2, 5, 10} and {(c[2], c[3]) for c in BITWISE} >= {(5, 0), (3, 2)} and col(4) == {13, 17}
    assert col(5) >= {1, 3, 70} and col(6) >= {1, 3, 16} and col(7) == {1, 40}
    assert any(c[8] and c[9] for c in BITWISE) and any(not c[8] and c[7] == 40 for c in BITWISE)
    assert col(10) == {_abi.HOLONOMIC, _abi.UNICYCLE}
    assert len({c[0] for c in BITWISE}) == len(BITWISE)


@pytest.mark.parametrize("cfg", list(reference_rollouts()), ids=lambda c: c[0])
def test_reference_rollout_is_finite_and_inside_the_bounds(cfg):
    """A condition on the inputs, checked where no GPU is needed: over the K steps of every configuration the host build's
    action is finite for every env, every robot stays inside the square the map covers, every env keeps adult_num rows
    (auto-reset restarts onto scenes of the same shape), and the env that starts inside its goal radius stands still."""
    tag, params, batch, pool, sd, K, flags = cfg
    out, state, where = oracle_rollout(tag, params, batch, sd, K, flags, pool)
    adult_num = sd["adult_encoder.0.weight"].shape[1] // 4
    assert out["robot_action_out"].shape == (K, batch.n, 2) and np.isfinite(out["robot_action_out"]).all(), tag
    assert (out["n_rows"] == adult_num).all(), tag
    assert where.shape == (K + 1, batch.n, 2) and (np.abs(where) < BOUND).all(), (tag, float(np.abs(where).max()))
    assert np.isfinite(out["reward"]).all() and np.isfinite(state["robot"]).all()
    if tag in [c[0] for c in BITWISE] and batch.n > 1:
        assert (out["robot_action_out"][0, ARRIVED_ENV] == 0).all() and out["robot_action_out"][0, 0].any(), tag
    if not flags and K == 40:
        assert out["done"][17:].all(), tag  # every env is past its time limit and keeps being stepped
    if flags and K >= 40:
        assert int(out["done"].sum()) > batch.n, tag  # restarts happen inside the window
