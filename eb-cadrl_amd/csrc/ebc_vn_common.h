// ebc_vn_common.h — types, fragment helpers, weight staging and the parking of group terms and row weights shared by the
// value-network kernels (ebc_value_net.h: the general two-layer block; ebc_vn_stream.h: the
// streamed blocks).  Conventions: the header of ebc_value_net.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebc_vn_layout.h"

namespace ebc {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float vn_f32x4 __attribute__((ext_vector_type(4)));
typedef vn_f32x4 __attribute__((address_space(3))) *LdsF4;  // explicit LDS pointers: no flat-address casts in the loops
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Frag2 {  // one operand fragment, split
  bf16x8 hi, lo;
};

__device__ __forceinline__ Frag2 split8(const float (&v)[8]) {
  Frag2 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f.hi[j] = (__bf16)v[j];
    f.lo[j] = (__bf16)(v[j] - (float)f.hi[j]);
  }
  return f;
}

// Two things the attention stack of the value network needs beyond a plain two-layer block.
//   row_bias [M / group_rows][H]: added to the hidden pre-activation of every row of a group (the
//     pair's mean-state term of attention layer 0, cat([h1, g]) without the concatenation);
//   final_w [O], final_b: a third layer with one output, y [M] = final_w . relu(out) + final_b,
//     worked out from the accumulators instead of storing out [M][O].
//   partial [ceil(M / 32)][3][O]: per 32-row tile, the weighted sums of its rows over each of the (at most three,
//     seg_rows >= 16) consecutive row groups of seg_rows rows it touches — sum_r row_weight[r] * y[r][:] (row_weight
//     NULL: 1) — so that a per-group mean (sarl.py:56-58) or attention-weighted sum (sarl.py:73-76) is the sum of
//     two or three of these (pair_combine_kernel) instead of a second pass over y; store_y == 0: y itself is not
//     written at all.  The sums are kept in float64 (products of two float32 are exact there, 18 of them add up
//     with 2^-53 relative error): whatever rows of a pair share a tile, whichever lanes hold them, the float32 the
//     combine step rounds to is the same — identical pairs at different places of the batch get identical results,
//     as with a serial row loop.
struct MlpExtra {
  const float *row_bias;
  int group_rows, H;
  const float *final_w;
  float final_b;
  const float *row_weight;
  double *partial;
  int seg_rows, store_y;
  // Round 3: activations handed from block to block ALREADY SPLIT and in fragment order.  frag_out: the output tiles
  // leave as the B fragments the next block's first layer multiplies — tile_frags() of the finished accumulators,
  // [row tile][output tile][k-step][hi, lo][lane] 16-byte pieces, the same 4 bytes per element as float32 rows —;
  // frag_in: the input IS such a tensor (X is not read): no row loads through an LDS transposition tile and no
  // per-lane split8 in the consumer's input phase.  A consumer of fragments has its first layer packed in accumulator
  // k order (ebc_mlp2_create_ex, EBC_MLP_IN_FRAGMENTS).
  const uint4 *frag_in;
  uint4 *frag_out;
};
#define EBC_VN_SEGS 3

// Packed layer: A fragments [out tile][in tile][k-step 0/1][hi, lo][lane][8 bf16] and the bias in
// accumulator order [out tile][lane half][16].
struct PackedLayer {
  const uint4 *frag;
  const float *bias;
  int in_tiles, out_tiles;
};

__device__ __forceinline__ f32x16 bias_tile(const PackedLayer &L, int t, int lane) {
  const float4 *b = reinterpret_cast<const float4 *>(L.bias + ((size_t)t * 2 + (lane >> 5)) * 16);
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = b[q];
    acc[4 * q] = v.x; acc[4 * q + 1] = v.y; acc[4 * q + 2] = v.z; acc[4 * q + 3] = v.w;
  }
  return acc;
}

// max(v, 0) for a finite v as ONE integer instruction on the bits (a negative float is a negative integer; -0 -> +0):
// fmaxf costs two, the first a canonicalisation of its operand that IEEE mode demands for signalling NaNs.  (A NaN with
// the sign bit clear stays a NaN where fmaxf gives 0: the blocks' values are finite or the result is garbage anyway.)
__device__ __forceinline__ float relu_bits(float v) {
  const int b = __float_as_int(v);
  return __int_as_float(b > 0 ? b : 0);
}

// the two B fragments (k-steps) a finished 32x32 tile offers to the next layer
__device__ __forceinline__ void tile_frags(const f32x16 &acc, bool relu, Frag2 (&out)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = relu ? relu_bits(acc[8 * s + j]) : acc[8 * s + j];
    out[s] = split8(v);
  }
}

// ---- pieces shared by the general block (ebc_value_net.h) and the streamed one (ebc_vn_stream.h) -------------------
typedef float __attribute__((address_space(3))) *LdsF;
typedef double __attribute__((address_space(3))) *LdsD;
constexpr int VN_PART = 64;  // uint4 per fragment half (hi or lo) = 1 KB

// One piece (1 KB) of packed weights, global -> LDS without registers (global_load_lds: a wave instruction).  As an asm
// statement: the builtin makes the compiler drain every outstanding load before the next LDS read (it cannot tell the
// buffers apart), which is the overlap the kernels are built for.  M0 = the wave-uniform LDS byte address; each lane
// supplies its source address.
__device__ __forceinline__ void lds_dma_piece(const uint4 *src, uint4 *dst, int lane) {
  unsigned keep;
  const uint4 *gsrc = src + lane;
  const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)dst);  // wave-uniform: a scalar register
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// The group terms (MlpExtra.row_bias) of the at most EBC_VN_GROUPS groups the wave's 32 rows (from row m0 on) belong to,
// parked in the wave's LDS rows `gt` (pitch EBC_VN_GROUP_PITCH, Hp = H rounded up to 4 floats each; groups past the last: 0).
__device__ __forceinline__ void park_group_terms(LdsF4 gt, const MlpExtra &ex, int m0, int M, int Hp, int lane) {
  const int first = m0 / ex.group_rows;
  const int groups_total = (M + ex.group_rows - 1) / ex.group_rows;
  for (int q = lane; q < EBC_VN_GROUPS * (Hp / 4); q += 64) {
    const int gq = q / (Hp / 4), c4 = q - gq * (Hp / 4);
    vn_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (first + gq < groups_total) v = *reinterpret_cast<const vn_f32x4 *>(ex.row_bias + (size_t)(first + gq) * ex.H + 4 * c4);
    gt[(gq * EBC_VN_GROUP_PITCH) / 16 + c4] = v;
  }
}

// The row weights of the pair sums (MlpExtra.partial), parked as float64 in the 16 spare bytes each 144-byte row of the
// wave's LDS tile `yt` has.  Row r's weight is parked TWICE, as the pair (w, 0) if the row belongs to the first group its
// 16-row half meets and (0, w) if to the second: the column walk of the tile epilogue is then two fused multiply-adds per row
// (the product of two float32 is exact in float64, so fma(w, y, a) IS a + w * y) instead of a multiply, two adds and four
// 32-bit selects.  Returns seg_lo: which of the tile's groups the first group of this lane's half is.
__device__ __forceinline__ int park_row_weights(LdsF4 yt, const MlpExtra &ex, int m0, int M, int lane) {
  const LdsD ytd = (LdsD)yt;
  if (lane < 32) {
    const int row = m0 + lane, hrow0 = m0 + (lane & 16);
    const int hnext = (hrow0 / ex.seg_rows + 1) * ex.seg_rows - hrow0;  // rows of this row's half before the next group starts
    const double w = row < M ? (ex.row_weight ? (double)ex.row_weight[row] : 1.0) : 0.0;
    const bool first = (lane & 15) < hnext;
    ytd[(lane * EBC_VN_XROW + 128) / 8] = first ? w : 0.0;
    ytd[(lane * EBC_VN_XROW + 136) / 8] = first ? 0.0 : w;
  }
  __builtin_amdgcn_wave_barrier();
  return (m0 + 16 * (lane >> 5)) / ex.seg_rows - m0 / ex.seg_rows;
}

template <int I>
struct IntC {  // a compile-time index as an argument (macro-free unrolling with constant register indices)
  static constexpr int value = I;
};

}  // namespace ebc
