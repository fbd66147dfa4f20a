"""ebc_step_k_world, the part that needs no GPU: the entry in the header, the bindings and the built library; the side
struct's layout against a compiled offsetof program; EbcStepKArgs and the ABI version as they were; what is refused
without a device; the Python surface of the host layer, the recorder and the tools."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest

from ebcsim import _abi, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ebcsim.h")
FIELDS = ["struct_size", "reserved", "robot", "ob"]


def test_entry_in_header_bindings_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+ebc_step_k_world\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 3 == len(_capi.SYMBOLS["ebc_step_k_world"][1])
    assert "EbcStepKArgs" in m.group(1) and "EbcStepKWorld" in m.group(1)
    assert _capi.SYMBOLS["ebc_step_k_world"][0] is C.c_int
    assert "#define EBC_ABI_VERSION 1" in text and _abi.ABI_VERSION == 1
    L = _capi.lib()  # raises if the product library lacks a symbol the bindings list
    assert hasattr(L, "ebc_step_k_world") and L.ebc_abi_version() == 1


def test_world_struct_layout_and_step_k_args_unchanged(tmp_path):
    S = _abi.EbcStepKWorld
    assert [f for f, _ in S._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu",sizeof(EbcStepKWorld),sizeof(EbcStepKArgs));\n%s\nprintf("\\n");return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu",offsetof(EbcStepKWorld,%s));' % f for f in FIELDS)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", exe], check=True, timeout=120)
    sizes = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert sizes == [C.sizeof(S), 112] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 24 and [getattr(S, f).offset for f in FIELDS] == [0, 4, 8, 16]
    assert C.sizeof(_abi.EbcStepKArgs) == 112 and len(_abi.EbcStepKArgs._fields_) == 17


def test_refused_without_a_device():
    """A null handle, whatever else is passed; and the side struct's own checks come before the handle's."""
    L = _capi.lib()
    a = _abi.EbcStepKArgs()
    a.struct_size = C.sizeof(a)
    a.K = 1
    buf = (C.c_double * 9)()
    w = _abi.EbcStepKWorld()
    w.struct_size = C.sizeof(w)
    w.robot = C.addressof(buf)
    assert L.ebc_step_k_world(None, C.addressof(a), C.addressof(w)) == _abi.ERR_INVALID
    assert b"null handle" in L.ebc_last_error()
    assert L.ebc_step_k_world(None, C.addressof(a), None) == _abi.ERR_INVALID
    assert b"world is NULL" in L.ebc_last_error()
    w.struct_size = C.sizeof(w) - 8
    assert L.ebc_step_k_world(None, C.addressof(a), C.addressof(w)) == _abi.ERR_INVALID
    assert b"EbcStepKWorld.struct_size" in L.ebc_last_error()
    w.struct_size, w.reserved = C.sizeof(w), 1
    assert L.ebc_step_k_world(None, C.addressof(a), C.addressof(w)) == _abi.ERR_INVALID
    assert b"EbcStepKWorld.reserved" in L.ebc_last_error()
    w.reserved, w.robot = 0, None
    assert L.ebc_step_k_world(None, C.addressof(a), C.addressof(w)) == _abi.ERR_INVALID
    assert b"both NULL" in L.ebc_last_error()


def test_python_surface():
    from ebcsim import sail_train, train
    from ebcsim.batched import BatchedEnv
    from ebcsim.record import EpisodeRecorder
    shapes = BatchedEnv._STEP_K_SHAPES(6, 4, 13)
    assert shapes["world_robot"] == ((6, 9), "float64") and shapes["world_ob"] == ((6, 4, 5), "float64")
    assert BatchedEnv._WORLD_KEYS == {"world_robot": "robot", "world_ob": "ob"}
    p = inspect.signature(sail_train.collect_sail_demos).parameters
    assert list(p) == ["env", "steps", "safety_space", "persistent_sim", "human_policy", "steps_per_call", "one_launch"]
    assert p["steps_per_call"].default is None and p["one_launch"].default is False
    p = inspect.signature(train.evaluate).parameters
    assert list(p)[-1] == "record" and p["record"].default is None
    assert list(inspect.signature(EpisodeRecorder.__init__).parameters) == ["self", "env", "steps"]
    for name in ("recording", "before_step", "episodes", "save"):
        assert callable(getattr(EpisodeRecorder, name))


@pytest.mark.parametrize("tool,options", [("train_sail.py", ("--demo-steps-per-call", "--demo-one-launch")),
                                          ("evaluate.py", ("--record",)), ("step_k_world_bench.py", ("--envs",))])
def test_tools_take_the_options(tool, options):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for o in options:
        assert o in r.stdout, o
