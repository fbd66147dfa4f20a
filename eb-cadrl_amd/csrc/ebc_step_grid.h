// ebc_step_grid.h — which envs / humans one-wave block `a` of the fused ORCA step launch (orca_step_kernel,
// ebc_kernels.h) owns, decided ONCE: the launcher (launch_orca_step, ebcsim.hip) takes the role sizes from here and
// the four roles their spans.  Plain C++17 constexpr, no HIP: tests/native/step_grid_host.cc compiles it with g++.
//
// Workgroups are dealt round-robin over the eight XCDs of the part (blocks a and a + 8 share an L2), and the L2s
// are not coherent with each other: a line that waves of two XCDs read is fetched through the fabric twice.  So
// the envs are cut into eight CLASSES of Ec = ceil(E / 8) consecutive envs, class c = [c Ec, min(E, (c + 1) Ec)),
// and every role deals its blocks to the classes by index: block r of a role has class r % 8 and rank r / 8, and
// owns the rank-th wave's worth of ITS class — envs for ENV / ROWS / STATE, flat humans (e N + i) for ORCA —
// clipped at the class's end, never at a neighbour's.  Every role takes 8 Q consecutive block indices (Q = the
// waves a full class needs), so every role's base is a multiple of 8 and every wave that reads or writes env e has
// the same a % 8.  Blocks past a class's end (the last class is short when 8 does not divide E, classes are empty
// when E < 8) own nothing.  Placement is only a matter of who fetches what: nothing in the hand-offs between the
// roles depends on where a block runs.
#pragma once

#define EBC_GRID_CLASSES 8    // XCDs of the part
#define EBC_GRID_WAVE 64      // lanes of a wave (EBC_WAVE)
#define EBC_GRID_ENV_EPW 16   // envs per ENV wave (EBC_WAVE / EBC_ENV_LANES)

namespace ebc {

// Units (envs, or flat humans) [first, end) of a block; nothing when end <= first.
struct StepSpan {
  unsigned first, end;
};

// Block r of a role whose classes own `per_class` units each out of `total`, `upw` units per wave.
// (32-bit: 7 per_class < total + 7 and rank upw < per_class + upw, with total < 2^31.)
constexpr StepSpan step_span(unsigned r, unsigned per_class, unsigned total, unsigned upw) {
  const unsigned c = r % EBC_GRID_CLASSES, q = r / EBC_GRID_CLASSES;
  const unsigned lo = c * per_class;
  const unsigned class_end = lo + per_class < total ? lo + per_class : total;  // below lo for an empty class
  const unsigned first = lo + q * upw;
  const unsigned end = first + upw < class_end ? first + upw : class_end;
  return StepSpan{first, end};
}

// The launch for E envs of N human slots and S static slots, `gs` lanes per ORCA group, with or without the ROWS role.
struct StepGridShape {
  unsigned ec;                   // envs per class
  unsigned orca_hpw, rows_epw, state_epw;  // humans per ORCA wave, envs per ROWS / STATE wave (ENV: EBC_GRID_ENV_EPW)
  unsigned long long env_blocks, orca_blocks, rows_blocks, state_blocks;  // 8 Q each, in this order in the grid

  constexpr unsigned long long total() const { return env_blocks + orca_blocks + rows_blocks + state_blocks; }
  constexpr bool fits() const { return total() < 2147483648ull; }  // the launcher refuses the others
  constexpr unsigned long long orca_base() const { return env_blocks; }
  constexpr unsigned long long rows_base() const { return env_blocks + orca_blocks; }
  constexpr unsigned long long state_base() const { return env_blocks + orca_blocks + rows_blocks; }
};

constexpr unsigned long long step_grid_role_blocks(unsigned long long per_class, unsigned upw) {
  return EBC_GRID_CLASSES * ((per_class + upw - 1) / upw);
}

constexpr StepGridShape step_grid_shape(int E, int N, int S, int gs, bool rows) {
  StepGridShape g{};
  const int R = N + S;
  g.ec = ((unsigned)E + EBC_GRID_CLASSES - 1) / EBC_GRID_CLASSES;
  g.orca_hpw = (unsigned)(EBC_GRID_WAVE / gs);
  g.rows_epw = R <= EBC_GRID_WAVE ? (unsigned)(EBC_GRID_WAVE / R) : 1u;  // more rows than lanes: an env per wave, in passes
  g.state_epw = (unsigned)(EBC_GRID_WAVE / N);
  g.env_blocks = step_grid_role_blocks(g.ec, EBC_GRID_ENV_EPW);
  g.orca_blocks = step_grid_role_blocks((unsigned long long)g.ec * (unsigned)N, g.orca_hpw);
  g.rows_blocks = rows ? step_grid_role_blocks(g.ec, g.rows_epw) : 0ull;
  g.state_blocks = step_grid_role_blocks(g.ec, g.state_epw);
  return g;
}

}  // namespace ebc
