// ebc_vn_layout.h — the workgroup and LDS layout of the general two-layer value-network block (mlp2_split_wg_kernel,
// ebc_value_net.h) for a pair of (input, output) tile counts, decided ONCE: the kernel takes its constants and its two
// run-time path conditions from here, the launcher (ebcsim_value_net.hip) the workgroup size, the LDS bytes and the
// refusal of the tile epilogue.  Plain C++17 constexpr, no HIP: tests/native/vn_layout_host.cc compiles it with g++ and
// prints the decisions over the whole lattice.
#pragma once

#include <stddef.h>

#define EBC_VN_XROW 144  // bytes per row of a wave's input transposition tile: 128 + 16 (conflict-free 16-byte reads)
#define EBC_VN_GROUPS 4         // group-term rows a wave parks in LDS (its 32 rows span at most that many groups)
#define EBC_VN_GROUP_PITCH 912  // bytes per parked row: 224 floats + 16

namespace ebc {

// A hidden tile's weights are two halves: its L1 row block (TI fragments, A) and its L2 column block (TO fragments, B),
// 4 KB per fragment (2 k-steps x hi / lo x 1 KB).  Three layouts:
//   full   A0 | B0 | A1 | B1, 4 waves: both halves double-buffered, where that fits a CU's LDS twice;
//   lean   A0 | B | A1, 4 waves: ONE slot for the L2 halves (staged at the start of the hidden phase of their own
//          tile), where the full layout does not fit twice and this one does: two independent 4-wave workgroups fill
//          each other's waits, which one lock-stepped 8-wave workgroup cannot;
//   full8  the full layout shared by 8 waves (two per SIMD with 256 registers each: measured faster than 4 waves with 512
//          for the widest shape, spills included), where neither fits twice.
struct VnLayout {
  int TI, TO;  // input / output tiles of 32

  static constexpr size_t HALF_CU = 78 * 1024;  // what a workgroup may take for two of them to live on a CU
  static constexpr size_t ONE_WG = 80 * 1024;   // a full layout above this is alone on its CU: 8 waves

  constexpr size_t full_bytes() const { return 2 * (size_t)(TI + TO) * 4096; }
  constexpr size_t lean_bytes() const { return (size_t)(2 * TI + TO) * 4096; }
  constexpr bool lean() const { return full_bytes() > HALF_CU && lean_bytes() <= HALF_CU; }
  constexpr int nw() const { return !lean() && full_bytes() > ONE_WG ? 8 : 4; }  // waves per workgroup, a 32-row tile each
  constexpr const char *name() const { return lean() ? "lean" : nw() == 8 ? "full8" : "full"; }

  // in uint4 (16 bytes), as the kernel indexes its LDS
  constexpr int a_size() const { return TI * 256; }
  constexpr int b_size() const { return TO * 256; }
  constexpr int per_u() const { return lean() ? (2 * a_size() + b_size() + 1) / 2 : a_size() + b_size(); }  // half the weight region
  // free for the waves' input tiles before the loop: from A1 on (nothing is staged there before the first barrier)
  constexpr int xoff() const { return a_size() + b_size(); }
  constexpr int xcap() const { return lean() ? a_size() : a_size() + b_size(); }

  // bytes: the weight region (behind the loop's last barrier also the waves' parked output tiles), then the hidden
  // layer's biases, then the waves' parked group terms
  constexpr size_t weight_bytes() const { return (size_t)per_u() * 2 * 16; }
  constexpr size_t epilogue_bytes() const { return weight_bytes(); }
  constexpr size_t group_offset(int hidden_tiles) const { return weight_bytes() + (size_t)hidden_tiles * 32 * 4; }
  constexpr size_t lds_bytes(int hidden_tiles, bool group_terms) const {
    return group_offset(hidden_tiles) + (group_terms ? (size_t)nw() * EBC_VN_GROUPS * EBC_VN_GROUP_PITCH : 0);
  }
  constexpr size_t wave_tiles_bytes() const { return (size_t)nw() * 32 * EBC_VN_XROW; }  // a transposition tile per wave

  // float32 rows [M][K0] reach the lanes through the waves' LDS tiles (16-byte rows, and the tiles fit) or by scalar loads
  constexpr bool rows_through_lds(int K0) const { return TI >= 2 && (K0 & 3) == 0 && wave_tiles_bytes() <= (size_t)xcap() * 16; }
  // the coalesced tile epilogue (row store through LDS, MlpExtra.partial, MlpExtra.frag_out) exists for this output width
  constexpr bool has_tile_epilogue(int O) const { return (O & 3) == 0 && wave_tiles_bytes() <= epilogue_bytes(); }
};

}  // namespace ebc
