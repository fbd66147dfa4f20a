// csrc/ebc_step_grid.h as the launcher and the four roles of orca_step_kernel compile it, enumerated on the host:
// every block of every role of every shape below is asked for its span, and the properties the kernel relies on
// are checked.  A finding prints a line and ends the program with status 1.  tests/test_step_grid_cpu.py builds
// and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_step_grid.h"

namespace {

const int kGroupSizes[] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32};  // ebcsim.hip's

long checked = 0;

[[noreturn]] void finding(const char *what, int E, int N, int S, int gs, bool rows, unsigned long long a) {
  std::printf("FINDING %s: E %d N %d S %d GS %d rows %d block %llu\n", what, E, N, S, gs, (int)rows, a);
  std::exit(1);
}

struct Shape {
  int E, N, S, gs;
  bool rows;
};

// One role: blocks [base, base + blocks), `total` units of which a class owns per_class, upw per wave;
// unit u belongs to env u / units_per_env.  Counts the owners of every unit and notes the class of every env.
void walk_role(const Shape &c, const char *role, unsigned long long base, unsigned long long blocks, unsigned per_class,
               unsigned total, unsigned upw, unsigned units_per_env, unsigned ec, std::vector<int> &env_class) {
  if (base % EBC_GRID_CLASSES || blocks % EBC_GRID_CLASSES) finding(role, c.E, c.N, c.S, c.gs, c.rows, base);
  std::vector<unsigned char> owners(total, 0);
  for (unsigned long long r = 0; r < blocks; ++r) {
    const unsigned long long a = base + r;
    const ebc::StepSpan s = ebc::step_span((unsigned)r, per_class, total, upw);
    if (s.end <= s.first) continue;  // owns nothing
    if (s.end - s.first > upw || s.end > total) finding("span too long", c.E, c.N, c.S, c.gs, c.rows, a);
    const unsigned cls = (unsigned)(a % EBC_GRID_CLASSES);
    if (s.first / per_class != cls || (s.end - 1) / per_class != cls) finding("span leaves its class", c.E, c.N, c.S, c.gs, c.rows, a);
    for (unsigned u = s.first; u < s.end; ++u) {
      if (owners[u]++) finding("unit owned twice", c.E, c.N, c.S, c.gs, c.rows, a);
      const unsigned e = u / units_per_env;
      if (e / ec != cls) finding("env outside the block's class", c.E, c.N, c.S, c.gs, c.rows, a);
      if (env_class[e] < 0) env_class[e] = (int)cls;
      if (env_class[e] != (int)cls) finding("owners of an env differ mod 8", c.E, c.N, c.S, c.gs, c.rows, a);
    }
  }
  for (unsigned u = 0; u < total; ++u)
    if (owners[u] != 1) finding("unit without an owner", c.E, c.N, c.S, c.gs, c.rows, u);
  ++checked;
}

void check(const Shape &c) {
  const ebc::StepGridShape g = ebc::step_grid_shape(c.E, c.N, c.S, c.gs, c.rows);
  if (!g.fits()) finding("refused", c.E, c.N, c.S, c.gs, c.rows, g.total());
  if (g.ec != (unsigned)(c.E + 7) / 8) finding("ec", c.E, c.N, c.S, c.gs, c.rows, g.ec);
  if (c.rows != (g.rows_blocks != 0)) finding("rows role", c.E, c.N, c.S, c.gs, c.rows, g.rows_blocks);
  // the order ENV, ORCA, ROWS, STATE: every producer index below every consumer index
  if (!(g.orca_base() == g.env_blocks && g.rows_base() == g.orca_base() + g.orca_blocks &&
        g.state_base() == g.rows_base() + g.rows_blocks && g.total() == g.state_base() + g.state_blocks))
    finding("role order", c.E, c.N, c.S, c.gs, c.rows, 0);
  if (g.env_blocks + g.orca_blocks > g.rows_base() || g.rows_base() > g.state_base())
    finding("producer above consumer", c.E, c.N, c.S, c.gs, c.rows, 0);
  std::vector<int> env_class((size_t)c.E, -1);
  const unsigned E = (unsigned)c.E, N = (unsigned)c.N;
  walk_role(c, "ENV", 0, g.env_blocks, g.ec, E, EBC_GRID_ENV_EPW, 1, g.ec, env_class);
  walk_role(c, "ORCA", g.orca_base(), g.orca_blocks, g.ec * N, E * N, g.orca_hpw, N, g.ec, env_class);
  if (c.rows) walk_role(c, "ROWS", g.rows_base(), g.rows_blocks, g.ec, E, g.rows_epw, 1, g.ec, env_class);
  walk_role(c, "STATE", g.state_base(), g.state_blocks, g.ec, E, g.state_epw, 1, g.ec, env_class);
}

}  // namespace

int main() {
  std::vector<int> Es;
  for (int e = 1; e <= 40; ++e) Es.push_back(e);
  for (int e : {50, 127, 128, 129, 1000, 4096, 4200, 16384}) Es.push_back(e);
  for (int E : Es)
    for (int N : {1, 5, 7, 10, 33})
      for (int S : {0, 3, 8, 95})
        for (int gs : kGroupSizes)
          if (gs >= N - 1)  // a lane per "other" human
            for (bool rows : {false, true}) check(Shape{E, N, S, gs, rows});
  // the launcher's refusal: the padded total, not the plain one, against 2^31 (64-bit sums)
  {
    const ebc::StepGridShape below = ebc::step_grid_shape(115000000, 33, 95, 32, true);
    const ebc::StepGridShape above = ebc::step_grid_shape(116000000, 33, 95, 32, true);
    if (!below.fits() || below.total() >= 2147483648ull) finding("refused below 2^31", 115000000, 33, 95, 32, true, below.total());
    if (above.fits() || above.total() < 2147483648ull) finding("accepted at 2^31", 116000000, 33, 95, 32, true, above.total());
    // the first total at or past 2^31 is refused and the last below it is not: found by bisection over E
    int lo = 115000000, hi = 116000000;
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      (ebc::step_grid_shape(mid, 33, 95, 32, true).total() < 2147483648ull ? lo : hi) = mid;
    }
    if (!ebc::step_grid_shape(lo, 33, 95, 32, true).fits() || ebc::step_grid_shape(hi, 33, 95, 32, true).fits())
      finding("refusal edge", hi, 33, 95, 32, true, ebc::step_grid_shape(hi, 33, 95, 32, true).total());
  }
  std::printf("group sizes");
  for (int gs : kGroupSizes) std::printf(" %d", gs);
  std::printf("\n");
  const ebc::StepGridShape b = ebc::step_grid_shape(4096, 10, 8, 9, true);
  std::printf("bench ec %u waves per class %llu %llu %llu %llu total %llu\n", b.ec, b.env_blocks / 8, b.orca_blocks / 8,
              b.rows_blocks / 8, b.state_blocks / 8, b.total());
  std::printf("ok %ld roles\n", checked);
  return 0;
}
