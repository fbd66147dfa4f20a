"""EBC_FLAG_ONE_LAUNCH in the bindings: the value the public header gives it, no collision with the other flags, and the
ABI version it was added under (additive: still 1)."""
import os
import py_compile
import re
import subprocess
import sys

import pytest

from ebcsim import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")


def _header_constants():
    with open(HEADER) as f:
        text = f.read()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(EBC_[A-Z_0-9]+)\s*=\s*(-?\d+)", text)}
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(EBC_[A-Z_0-9]+)\s+(-?\d+)\b", text)}
    return enums, defines


def test_one_launch_flag_matches_the_header():
    enums, _ = _header_constants()
    assert _abi.FLAG_ONE_LAUNCH == enums["EBC_FLAG_ONE_LAUNCH"] == 4
    assert _abi.FLAG_AUTO_RESET == enums["EBC_FLAG_AUTO_RESET"]
    assert _abi.FLAG_BORDER == enums["EBC_FLAG_BORDER"]


def test_flags_are_distinct_bits():
    flags = [_abi.FLAG_AUTO_RESET, _abi.FLAG_BORDER, _abi.FLAG_ONE_LAUNCH]
    assert all(f > 0 and f & (f - 1) == 0 for f in flags)
    assert len(set(flags)) == len(flags)


def test_abi_version_is_still_one():
    _, defines = _header_constants()
    assert defines["EBC_ABI_VERSION"] == 1 == _abi.ABI_VERSION


@pytest.mark.parametrize("tool", ["train_bench.py", "step_k_bench.py"])
def test_tools_with_the_one_launch_switch_parse_and_show_their_usage(tool, tmp_path):
    """No test imports these tools: a syntax error in one would go unseen.  Byte-compile them, and have them print their
    usage (argparse runs before anything that needs the library or a GPU)."""
    path = os.path.join(ROOT, "tools", tool)
    py_compile.compile(path, cfile=str(tmp_path / (tool + "c")), doraise=True)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    if tool == "train_bench.py":
        assert "--one-launch" in r.stdout
    else:
        assert "--outputs" in r.stdout and "--robots" in r.stdout
