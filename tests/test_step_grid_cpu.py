"""The grid of the fused ORCA step (csrc/ebc_step_grid.h: eight classes of envs, every role dealt to them by block
index mod 8), checked without a GPU: tests/native/step_grid_host.cc compiles the header with g++ as a program of its own
under -fsanitize=address,undefined and enumerates every block of every role over E in {1 .. 40, 50, 127, 128, 129, 1000,
4096, 4200, 16384} x N in {1, 5, 7, 10, 33} x S in {0, 3, 8, 95} x every instantiated group size >= N - 1, with and
without the ROWS role:

- every env has exactly one ENV, one ROWS and one STATE owner, every flat human exactly one ORCA group;
- no span crosses a class boundary, and all owners of an env have the same block index mod 8;
- every role's base is a multiple of 8, in the order ENV, ORCA, ROWS, STATE (producers below consumers);
- the padded total is refused from 2^31 on, and not below."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eb-cadrl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_step_grid_properties_over_the_lattice(tmp_path):
    exe = str(tmp_path / "step_grid_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "step_grid_host.cc"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) > 10000, lines[-3:]
    # the group sizes the program walks are the instantiated ones
    sizes = lines[-3].replace("group sizes ", "").split()
    assert "const int kGroupSizes[] = {%s};" % ", ".join(sizes) in _src("ebcsim.hip")
    # the headline launch: 4096 envs x 10 humans, 9-lane groups, 18 rows
    assert lines[-2] == "bench ec 512 waves per class 32 732 171 86 total 8168"


def test_the_launcher_and_the_roles_take_their_spans_from_the_header():
    kernels, host = _src("ebc_kernels.h"), _src("ebcsim.hip")
    assert kernels.count("step_span(") == 4  # ENV, ORCA, ROWS, STATE
    assert "block * epw" not in kernels and "block * HPW" not in kernels and "block * EPW" not in kernels
    assert "ebc::step_grid_shape(" in host and "shape.fits()" in host
    assert '#include "ebc_step_grid.h"' in kernels
    grid = _src("ebc_step_grid.h")
    assert "__global__" not in grid and "__device__" not in grid and "#include" not in grid  # plain C++
