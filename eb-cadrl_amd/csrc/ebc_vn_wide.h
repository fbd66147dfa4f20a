// ebc_vn_wide.h — the WIDE two-layer value-network block (ebc_mlp2_create_wide: K0, H, O up to 640, the widths of the
// reference's policy_x3 / policy_x4 networks): its kernels, and the host entries ebcsim_value_net.hip calls for a handle
// created wide (ebcsim_vn_wide.hip: a translation unit of its own, compiled beside the others).
//
// The general block (mlp2_split_wg_kernel, ebc_value_net.h) keeps the input fragments and the output accumulators of
// a row tile in registers: 7 + 7 tiles are 224 of its 256.  A wide block is therefore ONE single-layer kernel launched
// twice, with the hidden layer making a round trip through a scratch the handle owns:
//   layer 1: float32 rows [M][K0] -> hidden activations, biased (+ the group term), rectified and already split, in
//            the fragment layout blocks hand each other ([row tile][column tile][2 k-steps][hi, lo][64 lanes] x 16 B);
//   layer 2: those fragments -> rows [M][O], or through the one-output tail -> [M].
// Arithmetic: ebc_value_net.h's (x = hi + lo in bf16, hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, float32
// accumulators, bias / group term / ReLU in float32).  No atomics: every output has one owner and one order of sums.
//
// A workgroup = EBC_VNW_NW waves = that many 32-row tiles, which walk the layer's input tiles TOGETHER: the weight
// fragments of the current input tile for up to EBC_VNW_TG output tiles (4 KB each) are staged in LDS once per
// workgroup by global_load_lds and double-buffered — tile u + 1 arrives while tile u is multiplied.  Output tiles
// beyond EBC_VNW_TG are further passes: on blockIdx.y (a single layer recomputes nothing), or, for the one-output tail
// whose dot product crosses them, one after the other in the same workgroup.  The input of a k-step arrives per
// k-step, one tile ahead: float32 rows through the wave's LDS transposition tile (layer 1), 4 x 16 bytes per lane of
// the hidden fragments (layer 2).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebc_host.h"
#include "ebc_vn_common.h"

#define EBC_VNW_MAX 640                  // K0, H, O of a wide block: ebc_sarl_net_create_layers' limit
#define EBC_VNW_NW 8                     // waves per workgroup, a 32-row tile each
#define EBC_VNW_ROWS (32 * EBC_VNW_NW)   // rows per workgroup
#define EBC_VNW_TG 7                     // output tiles per pass: 112 accumulator registers
#define EBC_VNW_SLAB (1 << 17)           // rows per pair of launches: bounds the scratch (<= 320 MB per stream)
#define EBC_VNW_F32_KC 64                // input columns per LDS chunk of the float32 form
#define EBC_VNW_F32_TW 5                 // output tiles per wave of the float32 form (4 waves x 5 x 32 = 640)

namespace ebc {

struct WideArgs {
  const float *x;         // layer 1: rows [M][K]
  const uint4 *frag_in;   // layer 2: the hidden fragments
  uint4 *frag_out;        // layer 1: the hidden fragments
  float *y;               // layer 2: rows [M][N], or [M] behind the tail
  int M, K, N;            // rows of this launch, the layer's input and output widths
  int row0;               // the launch's first row in the caller's tensor (the group of a row: (row0 + m) / group_rows)
  const float *row_bias;  // layer 1: [groups][N] or NULL
  int group_rows;
  const float *final_w;   // layer 2: the one-output tail or NULL
  float final_b;
  int relu_out;
};

constexpr size_t vnw_weight_bytes() { return (size_t)2 * EBC_VNW_TG * 4096; }
constexpr size_t vnw_lds_bytes(bool first) { return vnw_weight_bytes() + (first ? (size_t)EBC_VNW_NW * 32 * EBC_VN_XROW : 0); }

template <bool FIRST>
__global__ __launch_bounds__(64 * EBC_VNW_NW) void wide_layer_kernel(PackedLayer L, WideArgs a) {
  extern __shared__ uint4 wlds[];  // weights: buffer 0 | buffer 1 (EBC_VNW_TG fragments each), then a transposition tile per wave
  constexpr int NW = EBC_VNW_NW, TG = EBC_VNW_TG, PART = VN_PART, BUF = TG * 4 * PART;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int tile = blockIdx.x * NW + wave, m0 = tile * 32, m = m0 + col;
  // a workgroup's last waves can lie past the last row tile: they stage weights and meet the barriers, read no input
  // and write nothing
  const bool tile_ok = m0 < a.M;
  const int Ti = L.in_tiles, To = L.out_tiles;
  const int passes = (To + TG - 1) / TG;
  // the input's width ends in the first half of its last tile: that tile's second k-step multiplies zeros
  const bool skip_last = a.K - 32 * (Ti - 1) <= 16;
  const LdsF4 xt = (LdsF4)(reinterpret_cast<unsigned char *>(wlds) + vnw_weight_bytes() + (size_t)wave * 32 * EBC_VN_XROW);
  const int piece = lane & 7, rsub = lane >> 3;
  const bool k16 = (a.K & 3) == 0;  // rows 16-byte aligned
  float fin = 0.0f;
  for (int pass = blockIdx.y; pass < passes; pass += gridDim.y) {
    const int t0 = pass * TG, nt = To - t0 < TG ? To - t0 : TG;
    auto stage = [&](int u, int buf) {  // fragment (t0 + t, u) = 4 pieces of 1 KB, contiguous
      for (int q = wave; q < nt * 4; q += NW)
        lds_dma_piece(L.frag + (((size_t)(t0 + (q >> 2)) * Ti + u) * 4 + (q & 3)) * PART, wlds + (size_t)buf * BUF + (size_t)q * PART, lane);
    };
    // the input of tile u, as it comes from memory: FIRST: four row pieces (8 consecutive lanes read one row's 128 bytes);
    // else the four 16-byte pieces of the lane's fragments
    vn_f32x4 pre[4];
    auto prefetch = [&](int u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pre[q] = vn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (!tile_ok) continue;
        if (FIRST) {
          const int r = rsub + 8 * q, kk = u * 32 + 4 * piece;
          if (m0 + r >= a.M) continue;
          const float *src = a.x + (size_t)(m0 + r) * a.K + kk;
          if (k16) {
            if (kk < a.K) pre[q] = *reinterpret_cast<const vn_f32x4 *>(src);
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (kk + c < a.K) pre[q][c] = src[c];
          }
        } else {
          const uint4 v = a.frag_in[(((size_t)tile * Ti + u) * 4 + q) * PART + lane];
          pre[q] = *reinterpret_cast<const vn_f32x4 *>(&v);
        }
      }
    };
    f32x16 out[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      if (t < nt) {
        out[t] = bias_tile(L, t0 + t, lane);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) out[t][r] = 0.0f;
      }
    }
    stage(0, 0);
    prefetch(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the compiler does not count the asm loads
    __syncthreads();
    for (int u = 0; u < Ti; ++u) {
      const int buf = u & 1;
      Frag2 x[2];
      if (FIRST) {
        // the wave parks the 32 x 32 block in its LDS tile (row pitch 144 B) and reads it back row per lane: element j
        // of k-step s is column 16 s + 8 half + j
#pragma unroll
        for (int q = 0; q < 4; ++q) xt[((rsub + 8 * q) * EBC_VN_XROW + piece * 16) / 16] = pre[q];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const vn_f32x4 p = xt[(col * EBC_VN_XROW + s * 64 + half * 32) / 16], q = xt[(col * EBC_VN_XROW + s * 64 + half * 32 + 16) / 16];
          const float v[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
          x[s] = split8(v);
        }
        __builtin_amdgcn_wave_barrier();  // the tile is rewritten by the next column block
      } else {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          x[s].hi = *reinterpret_cast<const bf16x8 *>(&pre[2 * s]);
          x[s].lo = *reinterpret_cast<const bf16x8 *>(&pre[2 * s + 1]);
        }
      }
      if (u + 1 < Ti) {  // the next tile's input and weights: in flight while this tile is multiplied
        prefetch(u + 1);
        stage(u + 1, buf ^ 1);
      }
      const uint4 *w = wlds + (size_t)buf * BUF + lane;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && u == Ti - 1 && skip_last) continue;
#pragma unroll
        for (int t = 0; t < TG; ++t) {
          if (t >= nt) continue;  // uniform
          const uint4 h = w[((t * 2 + s) * 2) * PART], l = w[((t * 2 + s) * 2 + 1) * PART];
          const bf16x8 whi = *reinterpret_cast<const bf16x8 *>(&h), wlo = *reinterpret_cast<const bf16x8 *>(&l);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, x[s].hi, out[t], 0, 0, 0);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, x[s].lo, out[t], 0, 0, 0);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, x[s].hi, out[t], 0, 0, 0);
        }
      }
      // everything issued above has landed and every wave is done with this tile's buffer
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    // ---- epilogue.  Register r of lane (col, half) of tile t: row m0 + col, unit 32 (t0 + t) + 8 (r >> 2) + 4 half + (r & 3)
    if (FIRST) {
      if (!tile_ok) continue;  // (uniform per wave; no barrier follows in this pass)
      const float *gb = (a.row_bias && m < a.M) ? a.row_bias + (size_t)((a.row0 + m) / a.group_rows) * a.N : nullptr;
      const bool n16 = (a.N & 3) == 0;
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        if (t >= nt) continue;
        if (gb) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int unit = (t0 + t) * 32 + 8 * g + 4 * half;
            if (n16) {
              if (unit < a.N) {
                const vn_f32x4 v = *reinterpret_cast<const vn_f32x4 *>(gb + unit);
#pragma unroll
                for (int c = 0; c < 4; ++c) out[t][4 * g + c] += v[c];
              }
            } else {
#pragma unroll
              for (int c = 0; c < 4; ++c)
                if (unit + c < a.N) out[t][4 * g + c] += gb[unit + c];
            }
          }
        }
        Frag2 of[2];
        tile_frags(out[t], true, of);
        uint4 *dst = a.frag_out + (((size_t)tile * To + t0 + t) * 4) * PART + lane;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          dst[(2 * s) * PART] = *reinterpret_cast<const uint4 *>(&of[s].hi);
          dst[(2 * s + 1) * PART] = *reinterpret_cast<const uint4 *>(&of[s].lo);
        }
      }
    } else if (a.final_w) {  // third layer with one output: the units this lane holds, pass after pass
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        if (t >= nt) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int unit = (t0 + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (unit < a.N) fin += a.final_w[unit] * relu_bits(out[t][r]);
        }
      }
    } else if (m < a.M) {
      const bool n16 = (a.N & 3) == 0;  // registers 4g .. 4g + 3 are four consecutive units: one 16-byte store
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        if (t >= nt) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int unit = (t0 + t) * 32 + 8 * g + 4 * half;
          vn_f32x4 v;
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = a.relu_out ? relu_bits(out[t][4 * g + c]) : out[t][4 * g + c];
          float *dst = a.y + (size_t)m * a.N + unit;
          if (n16) {
            if (unit < a.N) *reinterpret_cast<vn_f32x4 *>(dst) = v;
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (unit + c < a.N) dst[c] = v[c];
          }
        }
      }
    }
  }
  if (!FIRST && a.final_w) {
    fin += __shfl_xor(fin, 32, 64);
    if (m < a.M && half == 0) a.y[m] = fin + a.final_b;
  }
}

// ---- the float32 form (ebc_mlp2_forward_f32 on a wide handle): a single layer on v_mfma_f32_32x32x2_f32, per output
// one float32 chain with k ascending, launched twice with the hidden layer as float32 rows in the handle's scratch.
// For the few rows whose value decides an argmax: a workgroup is ONE 32-row tile, its four waves share the tile's
// output tiles (wave w: tiles w, w + 4, ...), the input tile waits transposed in LDS, EBC_VNW_F32_KC columns at a time,
// the weights come from L2 in the transposed layout [in][out padded to 64] (a wave's lanes: two 128-byte runs).
struct WideF32Layer {
  const float *wt;  // [in][out_pad]
  const float *b;   // [out_pad]
  int in, out, out_pad;
};
typedef float vnw_f32acc __attribute__((ext_vector_type(16)));

template <bool FIRST>
__global__ __launch_bounds__(256) void wide_f32_layer_kernel(WideF32Layer L, WideArgs a) {
  constexpr int KC = EBC_VNW_F32_KC, TW = EBC_VNW_F32_TW;
  __shared__ float xl[KC * 32];  // [k][row]
  __shared__ float finl[4 * 32];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, n = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.x * 32, row = m0 + n;
  const int K = L.in, N = L.out, P = L.out_pad, To = (N + 31) / 32;
  const bool k16 = (K & 3) == 0;
  vnw_f32acc out[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[i][r] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += KC) {
    __syncthreads();  // the previous chunk is no longer being read
    for (int idx = threadIdx.x; idx < (KC / 4) * 32; idx += 256) {  // thread -> (column quadruple c, row r): lanes = rows
      const int c = idx >> 5, r = idx & 31, k = k0 + 4 * c;
      float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (m0 + r < a.M) {
        const float *xr = a.x + (size_t)(m0 + r) * K + k;
        if (k16) {
          if (k < K) {
            const vn_f32x4 v = *reinterpret_cast<const vn_f32x4 *>(xr);
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k + j < K) q[j] = xr[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) xl[(4 * c + j) * 32 + r] = q[j];
    }
    __syncthreads();
    const int kend = K - k0 < KC ? K - k0 : KC;
    for (int kk = 0; kk < kend; kk += 2) {  // k-step (k, k + 1): lane half h takes column k + h
      const int k = k0 + kk + half;
      const float b = xl[(kk + half) * 32 + n];  // columns at or past K: zeros
      const float *wk = L.wt + (size_t)(k < K ? k : K - 1) * P + n;  // (a weight of the layer: finite, times 0)
      float w[TW];
#pragma unroll
      for (int i = 0; i < TW; ++i) w[i] = wave + 4 * i < To ? wk[(wave + 4 * i) * 32] : 0.0f;
#pragma unroll
      for (int i = 0; i < TW; ++i)
        if (wave + 4 * i < To) out[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[i], b, out[i], 0, 0, 0);
    }
  }
  // ---- epilogue: register r of lane (n, half) of tile t is row m0 + n, unit 32 t + 8 (r >> 2) + 4 half + (r & 3)
  const int gq = (FIRST && a.row_bias && row < a.M) ? (a.row0 + row) / a.group_rows : 0;
  const bool tail = !FIRST && a.final_w;
  const bool n16 = (N & 3) == 0;
  float fin = 0.0f;
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int t = wave + 4 * i;
    if (t >= To) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int unit0 = t * 32 + 8 * g + 4 * half;
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int unit = unit0 + c;
        v[c] = out[i][4 * g + c] + (unit < N ? L.b[unit] : 0.0f);
        if (FIRST && a.row_bias && unit < N && row < a.M) v[c] += a.row_bias[(size_t)gq * N + unit];
        if (FIRST || a.relu_out || tail) v[c] = v[c] > 0.0f ? v[c] : 0.0f;  // the one-output tail acts on relu(out)
        if (tail && unit < N) fin = __builtin_fmaf(a.final_w[unit], v[c], fin);
      }
      if (tail || row >= a.M) continue;
      float *dst = a.y + (size_t)row * N + unit0;
      if (n16) {
        if (unit0 < N) *reinterpret_cast<vn_f32x4 *>(dst) = vn_f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (unit0 + c < N) dst[c] = v[c];
      }
    }
  }
  if (tail) {  // uniform: the waves' shares of the dot product, added in wave order
    fin += __shfl_xor(fin, 32, 64);
    if (half == 0) finl[wave * 32 + n] = fin;
    __syncthreads();
    if (wave == 0 && half == 0 && row < a.M) {
      float s = 0.0f;
      for (int w = 0; w < 4 && w < To; ++w) s += finl[w * 32 + n];
      a.y[row] = s + a.final_b;
    }
  }
}

}  // namespace ebc

namespace ebc_host {

// What a wide handle carries beside the packed layers: the hidden layer's scratch, one per stream the block has run
// on (the chunks of a decision batch alternate between streams), grown on demand.
void *vn_wide_state_new();
void vn_wide_state_free(void *state);

struct VnWideCall {
  int device;
  hipStream_t st;
  int K0, H, O, M, relu_out;
  const float *x, *row_bias;
  int group_rows;
  const float *final_w;
  float final_b;
  float *y;
};
// the coarse form (ebc_mlp2_forward) and the float32 form (ebc_mlp2_forward_f32) of a wide block.  A captured stream is
// refused (EBC_ERR_UNSUPPORTED) when the call would have to allocate or raise a kernel's LDS limit.
int vn_wide_forward(void *state, const VnWideCall &c, const ebc::PackedLayer &L1, const ebc::PackedLayer &L2);
int vn_wide_forward_f32(void *state, const VnWideCall &c, const ebc::WideF32Layer &F1, const ebc::WideF32Layer &F2);

}  // namespace ebc_host
