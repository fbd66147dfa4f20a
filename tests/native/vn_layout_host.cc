// What csrc/ebc_vn_layout.h decides for the general two-layer value-network block, over the whole lattice of tile counts:
// the header the kernel and its launcher compile, built with g++ as a program of its own.  One line per (TI, TO):
//   TI TO class NW weight_bytes xcap_bytes epilogue_bytes lds_plain lds_group rows=<32 digits> epilogue=<3 digits>
// lds_plain / lds_group: the launch's dynamic LDS at 7 hidden tiles without / with parked group terms;
// rows: rows_through_lds(K0) for K0 = 32 (TI - 1) + 1 .. 32 TI; epilogue: has_tile_epilogue(O) at O = 32 TO,
// 32 (TO - 1) + 4 and 32 TO - 3.  tests/test_value_net_shapes_cpu.py holds the restatement in tests/value_net_cases.py to
// these lines.
#include <stdio.h>

#include "../../eb-cadrl_amd/csrc/ebc_vn_layout.h"

// the kernel's view of the same numbers: compile-time constants
static_assert(ebc::VnLayout{1, 1}.nw() == 4 && !ebc::VnLayout{1, 1}.lean() && !ebc::VnLayout{1, 1}.has_tile_epilogue(32), "1 + 1 tiles");
static_assert(ebc::VnLayout{7, 7}.nw() == 8 && ebc::VnLayout{7, 4}.lean(), "the attention block and mlp2 of SARL");

int main() {
  for (int TI = 1; TI <= 7; ++TI)
    for (int TO = 1; TO <= 7; ++TO) {
      const ebc::VnLayout ly{TI, TO};
      printf("%d %d %s %d %zu %zu %zu %zu %zu rows=", TI, TO, ly.name(), ly.nw(), ly.weight_bytes(), (size_t)ly.xcap() * 16,
             ly.epilogue_bytes(), ly.lds_bytes(7, false), ly.lds_bytes(7, true));
      for (int K0 = 32 * (TI - 1) + 1; K0 <= 32 * TI; ++K0) putchar(ly.rows_through_lds(K0) ? '1' : '0');
      printf(" epilogue=%d%d%d\n", (int)ly.has_tile_epilogue(32 * TO), (int)ly.has_tile_epilogue(32 * (TO - 1) + 4),
             (int)ly.has_tile_epilogue(32 * TO - 3));
    }
  printf("EBC_VN_XROW %d EBC_VN_GROUPS %d EBC_VN_GROUP_PITCH %d\n", EBC_VN_XROW, EBC_VN_GROUPS, EBC_VN_GROUP_PITCH);
  return 0;
}
