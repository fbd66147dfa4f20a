"""Each form of a gradient kernel that runs a chunk's states in passes keeps its own dynamic-LDS limit: the library raises
hipFuncAttributeMaxDynamicSharedMemorySize once per kernel instantiation and device and remembers what it raised, and a
memory shared between sarl_grad_kernel<true> and <false> (or lstm_grad_kernel's two) would leave the second form at the
64 KB default, where its launch is refused.  The attribute and the memory are process-wide, so the calls run in a fresh
child process (tests/grad_lds_limit_driver.py), which has launched neither form before."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grad_lds_limit_driver.py")


@pytest.mark.parametrize("kind", ["sarl", "lstm"])
def test_each_kernel_form_raises_its_own_lds_limit(kind):
    """Reference widths (SARL; LSTM-RL's ValueNetwork2), B = 1, one new network object: states_per_pass = 1 at
    R = grad_max_rows(1), the default call at R = grad_max_rows(), states_per_pass = 2 at R = grad_max_rows(2).  Every
    call returns EBC_OK (the child ends with status 1 at the first that does not) and gives the host build's bytes."""
    r = subprocess.run([sys.executable, DRIVER, kind], capture_output=True, text=True, timeout=120)
    assert r.stdout.strip(), r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0, (out, r.stderr[-3000:])
    assert [c["states_per_pass"] for c in out["calls"]] == [1, 0, 2]
    # at its row limit a call's LDS lies within one row (2.5 KB, 3.1 KB) of the 160 KB: far above the 64 KB a launch gets
    # without the attribute.  The limits at these widths are 64, 15, 32 (SARL) and 52, 12, 25 (LSTM-RL).
    assert all(c["R"] >= 12 for c in out["calls"]), out
    assert all(c["ok"] and c["same"] for c in out["calls"]), out
