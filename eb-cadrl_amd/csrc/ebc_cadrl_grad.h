// ebc_cadrl_grad.h — the CADRL value network's forward over every row of a chunk's states, the minimum over each state's
// rows, and the backward through each state's minimal row, as ONE kernel, and the small kernel that adds the chunks'
// partials: the arithmetic of ebc_cadrl_grad_rule.h, byte for byte.
//
// A workgroup of four waves owns one chunk of EBC_CADRL_GRAD_CHUNK consecutive states.
//   scan      (only when a state of the chunk has more than one row) the chunk's rows, flattened, in tiles of 16: the four
//             layers into LDS, layer 4's output into V[row]; then one thread per state takes min_rows and first_min_row.
//   keep      the 16 states' minimal rows once more, the same chains and so the same bytes, every layer into an LDS array
//             of its own (X0, A1, A2, A3): what the backward needs.  A state with one row has nothing to scan: its row 0.
//   layer     cadrl_layer: lane u owns unit u (u, u + 64, ...), a wave carries 4 rows of the tile; the weights W[k][u] are
//             read from the packed image in global memory (L2: 64 adjacent floats per wave and k), the inputs are LDS
//             broadcasts.
//   dW, db    cadrl_dw: a thread owns entries (k, u) of a layer; its chain runs over the chunk's live states ascending
//             from 0 and is stored ONCE into the chunk's partial.  A state that is not live is skipped by selection.
//   dx        cadrl_dx: a thread owns (state, input k); the chain over the layer's units runs ascending from 0; W[k][.]
//             are adjacent floats of the image, read 16 bytes at a time, the deltas 16-byte LDS reads.
// The partials [chunks][packed floats] are then added by grad_reduce (ebc_grad_common.h): one thread per weight, chunks
// ascending, in float64, rounded once.  No atomics, no polling: which workgroup runs a chunk, and when, cannot reach a sum.
//
// LDS, in floats: X0, SX [16][K0 padded]; A1, A2, A3 and D1, D2, D3 [16][units padded] (the deltas double as the scan's
// activations); V [16 R]; 16 outputs, 16 seeds and four small int arrays.  48 KB at the reference widths with one row per
// state, 56 KB at 128 rows; 115 KB at the widest network the entry takes: above the 64 KB a launch gets by default the
// entry raises the kernel's limit.  The weights (108 KB at the reference widths) stay in L2.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_grad_common.h"

#define EBC_CADRL_GRAD_WAVES 4

namespace ebc {

struct CadrlGradLaunch {
  const float *rows;          // [B][R][T]
  const long long *n_valid;   // [B] or nullptr = R
  const float *target;        // [B]
  const unsigned char *mask;  // [B] or nullptr
  float *value;               // [B] or nullptr
  int *min_row;               // [B] or nullptr
  float *partial;             // [chunks of this launch][D.floats]
  double *loss_part;          // [chunks of this launch]
  long long *count_part;      // [chunks of this launch]
  float grad_scale;
  int B, R;
  int chunk0;                 // the first chunk of this launch
  ebc_cadrl::GradDims D;
};

struct CadrlGradLds {
  float *X0, *SX, *A[3], *Dl[3], *V, *OUT, *SEED;
  int *LIVE, *N, *PICK, *PRE;
  int K0p;
};
__host__ __device__ inline size_t cadrl_grad_lds_floats(const ebc_cadrl::GradDims &D, int R) {
  constexpr int C = EBC_CADRL_GRAD_CHUNK;
  return (size_t)C * (2 * ebc_cadrl::pad4(D.K[0]) + 2 * (D.Op[0] + D.Op[1] + D.Op[2]) + R + 2 + 3) + 20;
}
__device__ __forceinline__ CadrlGradLds cadrl_grad_lds(float *p, const ebc_cadrl::GradDims &D, int R) {
  constexpr int C = EBC_CADRL_GRAD_CHUNK;
  CadrlGradLds L;
  L.K0p = ebc_cadrl::pad4(D.K[0]);
  L.X0 = p, p += C * L.K0p;
  L.SX = p, p += C * L.K0p;
  for (int l = 0; l < 3; ++l) L.A[l] = p, p += C * D.Op[l];
  for (int l = 0; l < 3; ++l) L.Dl[l] = p, p += C * D.Op[l];
  L.V = p, p += C * R;
  L.OUT = p, p += C;
  L.SEED = p, p += C;
  L.LIVE = reinterpret_cast<int *>(p), p += C;
  L.N = reinterpret_cast<int *>(p), p += C;
  L.PICK = reinterpret_cast<int *>(p), p += C;
  L.PRE = reinterpret_cast<int *>(p);  // C + 1 prefix sums of N
  return L;
}

// out[r][u] for r < nrows <= 16 and every unit u of the layer W[k][Op] | bias[Op]: grad_unit's chain, ReLU when asked
template <bool RELU>
__device__ __forceinline__ void cadrl_layer(const float *__restrict__ W, int K, int O, int Op, const float *in, int is, float *out, int os,
                                            int nrows) {
  constexpr int T = EBC_CADRL_GRAD_CHUNK / EBC_CADRL_GRAD_WAVES;
  const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * T;
  if (r0 >= nrows) return;
  const float *xr[T];
#pragma unroll
  for (int t = 0; t < T; ++t) xr[t] = in + (size_t)(r0 + t < nrows ? r0 + t : nrows - 1) * is;  // rows past the end: the last row, not stored
  for (int u = lane; u < O; u += 64) {
    float acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float w = W[(size_t)k * Op + u];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = ebc_cadrl::chain(xr[t][k], w, acc[t]);
    }
    const float b = W[(size_t)K * Op + u];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (r0 + t >= nrows) continue;
      const float y = acc[t] + b;
      out[(size_t)(r0 + t) * os + u] = RELU ? ebc_cadrl::grad_relu(y) : y;
    }
  }
}

// the four layers of nrows <= 16 rows x[r][0 .. K0) (LDS): the ReLU outputs into a1, a2, a3, layer 4's into out[r]
__device__ __forceinline__ void cadrl_forward_tile(const float *__restrict__ P, const ebc_cadrl::GradDims &D, const float *x, int xs, float *a1,
                                                   float *a2, float *a3, float *out, int nrows) {
  cadrl_layer<true>(P + D.at[0], D.K[0], D.O[0], D.Op[0], x, xs, a1, D.Op[0], nrows);
  __syncthreads();
  cadrl_layer<true>(P + D.at[1], D.K[1], D.O[1], D.Op[1], a1, D.Op[0], a2, D.Op[1], nrows);
  __syncthreads();
  cadrl_layer<true>(P + D.at[2], D.K[2], D.O[2], D.Op[2], a2, D.Op[1], a3, D.Op[2], nrows);
  __syncthreads();
  cadrl_layer<false>(P + D.at[3], D.K[3], D.O[3], D.Op[3], a3, D.Op[2], out, 1, nrows);
  __syncthreads();
}

// a layer's dW and db over the chunk's live states s < nc, ascending, into G (the layer's place in the chunk's partial,
// (K + 1) * Op floats): delta[s][u] at delta + s * ds, the layer's input x[s][k] at x + s * xs.  Pad entries get 0.
__device__ __forceinline__ void cadrl_dw(float *__restrict__ G, int K, int O, int Op, const float *delta, int ds, const float *x, int xs, int nc,
                                         const int *live) {
  constexpr int NT = 64 * EBC_CADRL_GRAD_WAVES;
  const int total = (K + 1) * Op;
  for (int idx = threadIdx.x; idx < total; idx += NT) {
    const int k = idx / Op, u = idx - k * Op;
    float acc = 0.0f;
    if (u < O) {
      if (k < K) {
        for (int s = 0; s < nc; ++s)
          if (live[s]) acc = ebc_cadrl::chain(delta[s * ds + u], x[s * xs + k], acc);
      } else {
        for (int s = 0; s < nc; ++s)
          if (live[s]) acc = acc + delta[s * ds + u];
      }
    }
    G[idx] = acc;
  }
}

// out[s][k] = relu_back(x[s][k], the chain over the layer's units u of W[k][u] * delta[s][u]) for the live states s < nc and
// every input k of the layer; x is the layer's input (the ReLU output the mask is taken from).  vec: delta rows are 16-byte
// aligned (ds a multiple of 4)
__device__ __forceinline__ void cadrl_dx(const float *__restrict__ W, int K, int O, int Op, const float *delta, int ds, const float *x, int xs,
                                         float *out, int os, int nc, const int *live, bool vec) {
  constexpr int NT = 64 * EBC_CADRL_GRAD_WAVES, C = EBC_CADRL_GRAD_CHUNK;
  for (int idx = threadIdx.x; idx < C * K; idx += NT) {
    const int k = idx / C, s = idx - k * C;
    if (s >= nc || !live[s]) continue;
    const float *w = W + (size_t)k * Op, *d = delta + s * ds;
    float acc = 0.0f;
    int u = 0;
    if (vec) {
      for (; u + 4 <= O; u += 4) {
        const float4 a = *reinterpret_cast<const float4 *>(w + u), b = *reinterpret_cast<const float4 *>(d + u);
        acc = ebc_cadrl::chain(a.x, b.x, acc);
        acc = ebc_cadrl::chain(a.y, b.y, acc);
        acc = ebc_cadrl::chain(a.z, b.z, acc);
        acc = ebc_cadrl::chain(a.w, b.w, acc);
      }
    }
    for (; u < O; ++u) acc = ebc_cadrl::chain(w[u], d[u], acc);
    out[s * os + k] = ebc_cadrl::grad_relu_back(x[s * xs + k], acc);
  }
}

__global__ __launch_bounds__(64 * EBC_CADRL_GRAD_WAVES) void cadrl_grad_kernel(const float *__restrict__ P, const CadrlGradLaunch a) {
  extern __shared__ float4 cadrl_grad_lds4[];
  constexpr int C = EBC_CADRL_GRAD_CHUNK, NT = 64 * EBC_CADRL_GRAD_WAVES;
  using namespace ebc_cadrl;
  const GradDims &D = a.D;
  const int tid = threadIdx.x, R = a.R, T = D.K[0];
  const CadrlGradLds L = cadrl_grad_lds(reinterpret_cast<float *>(cadrl_grad_lds4), D, R);
  const int K0p = L.K0p;
  const long long c0 = ((long long)a.chunk0 + blockIdx.x) * C;
  const int nc = a.B - c0 < C ? (int)(a.B - c0) : C;  // states of this chunk, >= 1
  float *const part = a.partial + (size_t)blockIdx.x * D.floats;

  // ---- the states' row counts, their prefix sums
  if (tid < C) L.N[tid] = tid < nc ? clamp_rows(a.n_valid ? a.n_valid[c0 + tid] : (long long)R, R) : 0;
  __syncthreads();
  if (tid == 0) {
    int q = 0;
    for (int s = 0; s < C; ++s) {
      L.PRE[s] = q;
      q += L.N[s];
    }
    L.PRE[C] = q;
  }
  __syncthreads();
  const int Q = L.PRE[C];
  bool scan = false;
  for (int s = 0; s < nc; ++s) scan = scan || L.N[s] > 1;  // workgroup-uniform

  // ---- scan: every row's value, then the minimum and its first row
  if (scan) {
    for (int q0 = 0; q0 < Q; q0 += C) {
      const int nt = Q - q0 < C ? Q - q0 : C;
      for (int i = tid; i < nt * T; i += NT) {
        const int r = i / T, k = i - r * T, q = q0 + r;
        int s = 0;
        while (q >= L.PRE[s + 1]) ++s;  // q < PRE[C]: ends at s < C
        L.SX[r * K0p + k] = a.rows[((size_t)(c0 + s) * R + (q - L.PRE[s])) * T + k];
      }
      __syncthreads();
      cadrl_forward_tile(P, D, L.SX, K0p, L.Dl[0], L.Dl[1], L.Dl[2], L.V + q0, nt);
    }
    if (tid < nc) {
      const float *v = L.V + L.PRE[tid];
      L.PICK[tid] = first_min_row(v, L.N[tid], min_rows(v, L.N[tid], 1));
    }
  } else if (tid < nc) {
    L.PICK[tid] = L.N[tid] >= 1 ? 0 : -1;
  }
  __syncthreads();

  // ---- keep: the minimal rows again, every layer's output kept
  for (int i = tid; i < nc * T; i += NT) {
    const int s = i / T, k = i - s * T, pick = L.PICK[s];
    L.X0[s * K0p + k] = pick >= 0 ? a.rows[((size_t)(c0 + s) * R + pick) * T + k] : 0.0f;  // a state without rows reads nothing
  }
  __syncthreads();
  cadrl_forward_tile(P, D, L.X0, K0p, L.A[0], L.A[1], L.A[2], L.OUT, nc);

  // ---- the outputs of the forward and the seeds, a thread per state; the chunk's loss in state order: thread 0's
  double *const state_loss = reinterpret_cast<double *>(L.SX);  // the scan is over: C doubles fit its C * K0p >= 64 floats
  if (tid < nc) {
    const long long b = c0 + tid;
    const float val = grad_value(L.OUT[tid], L.N[tid]);
    if (a.value) a.value[b] = val;
    if (a.min_row) a.min_row[b] = L.PICK[tid];
    const bool live = grad_live(!a.mask || a.mask[b] != 0, L.N[tid]);
    L.LIVE[tid] = live ? 1 : 0;
    if (live) {
      const float d = grad_diff(val, a.target[b]);
      state_loss[tid] = grad_loss(d);
      L.SEED[tid] = a.grad_scale * d;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double loss = 0.0;
    long long count = 0;
    for (int s = 0; s < nc; ++s) {
      if (!L.LIVE[s]) continue;
      loss = loss + state_loss[s];
      count += 1;
    }
    a.loss_part[blockIdx.x] = loss;
    a.count_part[blockIdx.x] = count;
  }

  // ---- backward
  cadrl_dw(part + D.at[3], D.K[3], D.O[3], D.Op[3], L.SEED, 1, L.A[2], D.Op[2], nc, L.LIVE);
  cadrl_dx(P + D.at[3], D.K[3], D.O[3], D.Op[3], L.SEED, 1, L.A[2], D.Op[2], L.Dl[2], D.Op[2], nc, L.LIVE, false);
  __syncthreads();
  cadrl_dw(part + D.at[2], D.K[2], D.O[2], D.Op[2], L.Dl[2], D.Op[2], L.A[1], D.Op[1], nc, L.LIVE);
  cadrl_dx(P + D.at[2], D.K[2], D.O[2], D.Op[2], L.Dl[2], D.Op[2], L.A[1], D.Op[1], L.Dl[1], D.Op[1], nc, L.LIVE, true);
  __syncthreads();
  cadrl_dw(part + D.at[1], D.K[1], D.O[1], D.Op[1], L.Dl[1], D.Op[1], L.A[0], D.Op[0], nc, L.LIVE);
  cadrl_dx(P + D.at[1], D.K[1], D.O[1], D.Op[1], L.Dl[1], D.Op[1], L.A[0], D.Op[0], L.Dl[0], D.Op[0], nc, L.LIVE, true);
  __syncthreads();
  cadrl_dw(part + D.at[0], D.K[0], D.O[0], D.Op[0], L.Dl[0], D.Op[0], L.X0, K0p, nc, L.LIVE);
}

}  // namespace ebc
