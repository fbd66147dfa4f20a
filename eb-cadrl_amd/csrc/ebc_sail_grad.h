// ebc_sail_grad.h — the SAIL network's forward with every activation kept on chip, then its backward, as ONE kernel, and
// the small kernel that adds the chunks' partials: the arithmetic of ebc_sail_grad_rule.h, byte for byte.
//
// A workgroup of eight waves owns one chunk of EBC_SAIL_GRAD_CHUNK consecutive envs and walks it in groups of
// grad_group_envs(N) whole envs (at most EBC_SAIL_GRAD_ROWS adult rows).  Per group:
//   forward   sail_layer of ebc_sail.h (lane u owns unit u, a wave carries EBC_SAIL_T rows), every layer into an LDS
//             array of its own: the chains are ebc_sail_forward's.
//   dx        grad_dx: lane k owns input k of a layer, a wave carries 4 rows; the chain over the layer's units o runs
//             ascending from 0; the weights W[k][0 .. 64) are 64 adjacent floats of the packed image, read 16 bytes at a
//             time, the deltas 16-byte LDS broadcasts.
//   dW, db    grad_dw: lane o owns unit o, a wave takes 4 inputs k at a time; the chain runs over the group's live rows
//             ascending and CONTINUES the chunk's partial in global memory: the same thread owns the same entries in
//             every group, reads what it wrote itself and stores it back.  A row of an env with w_e = 0 is skipped by a
//             (workgroup-uniform) selection, never multiplied by 0.
// The partials [chunks][packed_floats] are then added by grad_reduce<false> (ebc_grad_common.h): one thread per weight, chunks
// ascending, in float64, rounded once.  No atomics, no polling: which workgroup runs a chunk, and when, cannot reach a sum.
//
// LDS, in floats (rows = G * N, KX = max(4 N, 64)): X [rows][KX]; A1, A2, CAT, EMB, P1, FP, Q1 [rows][64] the layers'
// outputs; D0, D1 [rows][64] the deltas' ping-pong; per row the frame [4], logit, score, dscore, dlogit and the live flag;
// per env 9 arrays of 64, JIN and DJIN [128], the inputs and the live flag.  96 KB at 30 rows of 5 adults, 95 KB at 32 rows
// of 32, 110 KB at the most (32 rows of 4): above the 64 KB a launch gets by default, so the entry raises the kernel's limit.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_sail.h"
#include "ebc_grad_common.h"
#include "ebc_sail_grad_rule.h"

#define EBC_SAIL_GRAD_WAVES 8

namespace ebc {

struct SailGradLaunch {
  const double *robot;        // [E][9]
  const double *ob;           // [E][R][5]
  const long long *n_rows;    // [E] or nullptr = N
  const double *target;       // [E][2]
  const unsigned char *mask;  // [E] or nullptr
  double *action;             // [E][2] or nullptr
  float *partial;             // [chunks of this launch][packed_floats]
  double *loss_part;          // [chunks of this launch]
  long long *count_part;      // [chunks of this launch]
  float grad_scale;
  int E, R, N;
  int chunk0;                 // the first chunk of this launch
};

struct SailGradLds {
  float *X, *A1, *A2, *CAT, *EMB, *P1, *FP, *Q1, *D0, *D1, *FR, *LG, *SC, *DS, *DL;
  float *RIN, *TIN, *R1, *R2, *T1, *JIN, *FJ, *PL, *DA, *DFJ, *DJIN, *DT1, *DR2, *DR1;
  int *LIVE_ROW, *LIVE;
  double *LOSS;      // the chunk's loss so far and, behind it, its live envs: thread 0's
  long long *COUNT;
  int KX;
};
__host__ __device__ inline size_t sail_grad_lds_floats(int G, int N) {
  const int rows = G * N, KX = 4 * N > 64 ? 4 * N : 64;
  return (size_t)rows * (KX + 9 * 64 + 4 + 4 + 1) + (size_t)G * (9 * 64 + 2 * 128 + 4 + 4 + 4 + 1) + 4;
}
__device__ __forceinline__ SailGradLds sail_grad_lds(float *base, int G, int N) {
  constexpr int H = EBC_SAIL_HIDDEN;
  const size_t rows = (size_t)G * N;
  SailGradLds L;
  L.KX = 4 * N > 64 ? 4 * N : 64;
  L.LOSS = reinterpret_cast<double *>(base);
  L.COUNT = reinterpret_cast<long long *>(base) + 1;
  float *p = base + 4;
  L.X = p, p += rows * L.KX;
  L.A1 = p, p += rows * H;
  L.A2 = p, p += rows * H;
  L.CAT = p, p += rows * H;
  L.EMB = p, p += rows * H;
  L.P1 = p, p += rows * H;
  L.FP = p, p += rows * H;
  L.Q1 = p, p += rows * H;
  L.D0 = p, p += rows * H;
  L.D1 = p, p += rows * H;
  L.FR = p, p += rows * 4;
  L.RIN = p, p += G * 4;
  L.TIN = p, p += G * 4;
  L.DA = p, p += G * 4;
  L.R1 = p, p += G * H;
  L.R2 = p, p += G * H;
  L.T1 = p, p += G * H;
  L.JIN = p, p += G * 2 * H;
  L.FJ = p, p += G * H;
  L.PL = p, p += G * H;
  L.DFJ = p, p += G * H;
  L.DJIN = p, p += G * 2 * H;
  L.DT1 = p, p += G * H;
  L.DR2 = p, p += G * H;
  L.DR1 = p, p += G * H;
  // the scalar-per-row arrays last: 4 * rows floats + rows ints, then G ints
  L.LG = p, p += rows;
  L.SC = p, p += rows;
  L.DS = p, p += rows;
  L.DL = p, p += rows;
  L.LIVE_ROW = reinterpret_cast<int *>(p), p += rows;
  L.LIVE = reinterpret_cast<int *>(p);
  return L;
}

enum { GRAD_DX_RAW = 0, GRAD_DX_RELU = 1, GRAD_DX_ADD_RELU = 2, GRAD_DX_JOINT = 3 };

// out[r][k] from dx[r][k] = the chain over the units o of layer l of W[k][o] * delta[r][o], for r < nrows and every
// input k of the layer; x[r][k] is the layer's input (the ReLU output the mask is taken from):
//   RAW       out = dx                          RELU      out = x > 0 ? dx : 0
//   ADD_RELU  out = x > 0 ? out + dx : 0        JOINT     RELU for k < 64 (the task half), RAW from there (the crowd half)
// A function of its own, not inlined: inlined thirteen times beside the forward's layers and the dW chains it costs the
// group's body its registers (spills), and the kernel ran 15 % slower (profiles/sail_train.txt).
template <int MODE, int WAVES>
__device__ __noinline__ void grad_dx(const float *__restrict__ P, int N, int l, const float *d, int ds, const float *x, int xs,
                                        float *out, int os, int nrows) {
  constexpr int T = 4, H = EBC_SAIL_HIDDEN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = ebc_sail::layer_in(l, N), O = ebc_sail::layer_out(l);
  for (int k = lane; k < K; k += 64) {
    const float *W = P + ebc_sail::layer_offset(l, N) + (size_t)k * H;
    for (int r0 = wave * T; r0 < nrows; r0 += WAVES * T) {
      float acc[T];
      const float *dr[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        acc[t] = 0.0f;
        const int r = r0 + t < nrows ? r0 + t : nrows - 1;  // a tile's rows past the end read the last row and store nothing
        dr[t] = d + (size_t)r * ds;
      }
      if (O >= 4) {  // 32 or 64 units
        for (int o4 = 0; o4 < O / 4; ++o4) {
          const float4 w = reinterpret_cast<const float4 *>(W)[o4];
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const float4 v = reinterpret_cast<const float4 *>(dr[t])[o4];
            acc[t] = fmaf(w.x, v.x, acc[t]);
            acc[t] = fmaf(w.y, v.y, acc[t]);
            acc[t] = fmaf(w.z, v.z, acc[t]);
            acc[t] = fmaf(w.w, v.w, acc[t]);
          }
        }
      } else {
        for (int o = 0; o < O; ++o) {
          const float w = W[o];
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] = fmaf(w, dr[t][o], acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (r0 + t >= nrows) continue;
        const float xv = x[(size_t)(r0 + t) * xs + k];
        float *o = out + (size_t)(r0 + t) * os + k;
        if (MODE == GRAD_DX_RAW) *o = acc[t];
        else if (MODE == GRAD_DX_RELU) *o = ebc_sail::relu_back(xv, acc[t]);
        else if (MODE == GRAD_DX_ADD_RELU) *o = ebc_sail::relu_back(xv, *o + acc[t]);
        else *o = k < H ? ebc_sail::relu_back(xv, acc[t]) : acc[t];
      }
    }
  }
}

// The chains of layer l's dW and db continued over the rows r < nrows with live[r / per] != 0, ascending, in the chunk's
// partial G (packed layout): lane o owns unit o, the waves share the tiles of 4 inputs (the bias is one tile more).
// `first`: the chains start here (nothing is read).  Pad entries (units past the layer's width) are stored as 0.
template <int WAVES>
__device__ __forceinline__ void grad_dw(float *__restrict__ G, int N, int l, const float *d, int ds, const float *x, int xs, int nrows,
                                        const int *live, int per, bool first, int first_wave) {
  constexpr int H = EBC_SAIL_HIDDEN;
  const int lane = threadIdx.x & 63, wave = ((threadIdx.x >> 6) - first_wave + WAVES) % WAVES;
  const int K = ebc_sail::layer_in(l, N), O = ebc_sail::layer_out(l);
  float *g = G + ebc_sail::layer_offset(l, N) + lane;
  const bool unit = lane < O;
  for (int t = wave; t <= K / 4; t += WAVES) {  // every K is a multiple of 4
    if (t < K / 4) {
      float *g4 = g + (size_t)(4 * t) * H;
      float a0 = first ? 0.0f : g4[0], a1 = first ? 0.0f : g4[H], a2 = first ? 0.0f : g4[2 * H], a3 = first ? 0.0f : g4[3 * H];
      for (int r = 0; r < nrows; ++r) {
        if (!live[r / per]) continue;
        const float dv = unit ? d[(size_t)r * ds + lane] : 0.0f;
        const float4 v = *reinterpret_cast<const float4 *>(x + (size_t)r * xs + 4 * t);
        a0 = fmaf(dv, v.x, a0);
        a1 = fmaf(dv, v.y, a1);
        a2 = fmaf(dv, v.z, a2);
        a3 = fmaf(dv, v.w, a3);
      }
      g4[0] = unit ? a0 : 0.0f;
      g4[H] = unit ? a1 : 0.0f;
      g4[2 * H] = unit ? a2 : 0.0f;
      g4[3 * H] = unit ? a3 : 0.0f;
    } else {
      float *gb = g + (size_t)K * H;
      float a = first ? 0.0f : *gb;
      for (int r = 0; r < nrows; ++r) {
        if (!live[r / per]) continue;
        a = a + (unit ? d[(size_t)r * ds + lane] : 0.0f);
      }
      *gb = unit ? a : 0.0f;
    }
  }
}

// One group of `ne` whole envs from env e0 of a chunk: the forward, the outputs, the loss (thread 0's) and the backward
// into the chunk's partial.  A function of its own, called once per group: inlined into the chunk's loop, everything that
// does not change from group to group (some forty address computations per lane) is hoisted out of the loop and spilled.
__device__ __noinline__ void sail_grad_group(const float *__restrict__ P, const SailGradLaunch a, float *__restrict__ part, long long e0, int ne,
                                             bool first) {
  extern __shared__ float4 sail_grad_lds4[];
  constexpr int H = EBC_SAIL_HIDDEN, LOC = EBC_SAIL_LOCAL, WAVES = EBC_SAIL_GRAD_WAVES, NT = 64 * WAVES;
  using namespace ebc_sail;
  const int N = a.N, tid = threadIdx.x, lane = tid & 63, rows = ne * N;
  const SailGradLds L = sail_grad_lds(reinterpret_cast<float *>(sail_grad_lds4), grad_group_envs(N), N);
  const int KX = L.KX;
  {
    __syncthreads();  // the previous group's last readers are done
    // the casts, the live flags
    for (int g = tid; g < ne; g += NT) {
      const long long e = e0 + g;
      float rv[6], task[4];
      robot_vectors(a.robot + (size_t)e * 9, rv, task);
      for (int c = 0; c < 4; ++c) {
        L.RIN[4 * g + c] = rv[c];
        L.TIN[4 * g + c] = task[c];
      }
      L.LIVE[g] = grad_live(a.robot + (size_t)e * 9, a.n_rows ? a.n_rows[e] : (long long)N, N, !a.mask || a.mask[e] != 0) ? 1 : 0;
    }
    for (int q = tid; q < rows * 4; q += NT) {
      const int r = q >> 2, c = q & 3, g = r / N, i = r - g * N;
      L.FR[q] = (float)a.ob[((size_t)(e0 + g) * a.R + i) * 5 + c];
    }
    __syncthreads();
    for (int q = tid; q < rows * 4 * N; q += NT) {
      const int r = q / (4 * N), k = q - r * 4 * N, g = r / N, i = r - g * N;
      L.X[(size_t)r * KX + k] = frame_input(L.FR + (size_t)g * N * 4, i, k);
    }
    __syncthreads();
    // ---- forward: ebc_sail.h's layers, each into its own array
    sail_layer<true, WAVES>(P, N, ADULT0, L.X, KX, L.A1, H, 0, rows, 0);
    sail_layer<true, WAVES>(P, N, ROBOT0, L.RIN, 4, L.R1, H, 0, ne, WAVES - 1);
    sail_layer<true, WAVES>(P, N, TASK0, L.TIN, 4, L.T1, H, 0, ne, WAVES - 2);
    __syncthreads();
    sail_layer<true, WAVES>(P, N, ADULT2, L.A1, H, L.A2, H, 0, rows, 0);
    sail_layer<true, WAVES>(P, N, ROBOT2, L.R1, H, L.R2, H, 0, ne, WAVES - 1);
    sail_layer<true, WAVES>(P, N, TASK2, L.T1, H, L.JIN, 2 * H, 0, ne, WAVES - 2);
    __syncthreads();
    sail_layer<true, WAVES>(P, N, HEAD, L.A2, H, L.CAT, H, LOC, rows, 0);
    for (int q = tid; q < rows * LOC; q += NT) {
      const int r = q / LOC, u = q - r * LOC;
      L.CAT[(size_t)r * H + u] = L.R2[(r / N) * H + u];
    }
    __syncthreads();
    sail_layer<true, WAVES>(P, N, EMBED, L.CAT, H, L.EMB, H, 0, rows, 0);
    __syncthreads();
    sail_layer<true, WAVES>(P, N, PAIR0, L.EMB, H, L.P1, H, 0, rows, 0);
    sail_layer<true, WAVES>(P, N, ATT0, L.EMB, H, L.Q1, H, 0, rows, 0);
    __syncthreads();
    sail_layer<false, WAVES>(P, N, PAIR2, L.P1, H, L.FP, H, 0, rows, 0);
    sail_layer<false, WAVES>(P, N, ATT2, L.Q1, H, L.LG, 1, 0, rows, 0);
    __syncthreads();
    for (int g = tid >> 6; g < ne; g += WAVES) {
      float *score = L.SC + g * N;  // every lane writes the same values
      softmax(L.LG + g * N, 1, N, score);
      float acc = 0.0f;
      for (int j = 0; j < N; ++j) acc = fmaf(L.FP[(size_t)(g * N + j) * H + lane], score[j], acc);
      L.JIN[g * 2 * H + H + lane] = acc;
    }
    __syncthreads();
    sail_layer<true, WAVES>(P, N, JOINT, L.JIN, 2 * H, L.FJ, H, 0, ne, 0);
    __syncthreads();
    sail_layer<false, WAVES>(P, N, PLANNER, L.FJ, H, L.PL, H, 0, ne, 0);
    __syncthreads();
    // ---- the outputs of the forward, the loss and the seed
    for (int q = tid; q < ne * 2; q += NT) {
      const int g = q >> 1, c = q & 1;
      const long long e = e0 + g;
      if (a.action) {
        const bool rows_ok = !a.n_rows || a.n_rows[e] == (long long)N;
        a.action[(size_t)e * 2 + c] = action_of(L.PL[g * H + c], arrived(a.robot + (size_t)e * 9), rows_ok);
      }
      L.DA[4 * g + c] = L.LIVE[g] ? a.grad_scale * grad_diff(L.PL[g * H + c], a.target[(size_t)e * 2 + c]) : 0.0f;
    }
    for (int r = tid; r < rows; r += NT) L.LIVE_ROW[r] = L.LIVE[r / N];
    if (tid == 0) {
      double loss = *L.LOSS;
      long long count = *L.COUNT;
      for (int g = 0; g < ne; ++g) {
        if (!L.LIVE[g]) continue;
        const long long e = e0 + g;
        loss = loss + grad_loss(grad_diff(L.PL[g * H], a.target[(size_t)e * 2]), grad_diff(L.PL[g * H + 1], a.target[(size_t)e * 2 + 1]));
        count += 1;
      }
      *L.LOSS = loss;
      *L.COUNT = count;
    }
    __syncthreads();
    // ---- backward
    grad_dw<WAVES>(part, N, PLANNER, L.DA, 4, L.FJ, H, ne, L.LIVE, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, PLANNER, L.DA, 4, L.FJ, H, L.DFJ, H, ne);
    __syncthreads();
    grad_dw<WAVES>(part, N, JOINT, L.DFJ, H, L.JIN, 2 * H, ne, L.LIVE, 1, first, 0);
    grad_dx<GRAD_DX_JOINT, WAVES>(P, N, JOINT, L.DFJ, H, L.JIN, 2 * H, L.DJIN, 2 * H, ne);
    __syncthreads();
    // the crowd sum and the softmax; the task encoder beside them
    for (int r = tid; r < rows; r += NT) {
      const float *dC = L.DJIN + (r / N) * 2 * H + H, *fp = L.FP + (size_t)r * H;
      float s = 0.0f;
      for (int u = 0; u < H; ++u) s = fmaf(dC[u], fp[u], s);
      L.DS[r] = s;
    }
    for (int q = tid; q < rows * H; q += NT) {
      const int r = q / H, u = q - r * H;
      L.D0[q] = L.DJIN[(r / N) * 2 * H + H + u] * L.SC[r];  // dFP
    }
    grad_dw<WAVES>(part, N, TASK2, L.DJIN, 2 * H, L.T1, H, ne, L.LIVE, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, TASK2, L.DJIN, 2 * H, L.T1, H, L.DT1, H, ne);
    __syncthreads();
    for (int g = tid; g < ne; g += NT) {
      float dot = 0.0f;
      for (int j = 0; j < N; ++j) dot = fmaf(L.SC[g * N + j], L.DS[g * N + j], dot);
      for (int j = 0; j < N; ++j) L.DL[g * N + j] = softmax_back(L.SC[g * N + j], L.DS[g * N + j], dot);
    }
    grad_dw<WAVES>(part, N, TASK0, L.DT1, H, L.TIN, 4, ne, L.LIVE, 1, first, WAVES - 1);
    grad_dw<WAVES>(part, N, PAIR2, L.D0, H, L.P1, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, PAIR2, L.D0, H, L.P1, H, L.D1, H, rows);
    __syncthreads();
    grad_dw<WAVES>(part, N, PAIR0, L.D1, H, L.EMB, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_RAW, WAVES>(P, N, PAIR0, L.D1, H, L.EMB, H, L.D0, H, rows);  // the pairwise path of dEmb
    __syncthreads();
    grad_dw<WAVES>(part, N, ATT2, L.DL, 1, L.Q1, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, ATT2, L.DL, 1, L.Q1, H, L.D1, H, rows);
    __syncthreads();
    grad_dw<WAVES>(part, N, ATT0, L.D1, H, L.EMB, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_ADD_RELU, WAVES>(P, N, ATT0, L.D1, H, L.EMB, H, L.D0, H, rows);  // + the attention path, the ReLU
    __syncthreads();
    grad_dw<WAVES>(part, N, EMBED, L.D0, H, L.CAT, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, EMBED, L.D0, H, L.CAT, H, L.D1, H, rows);
    __syncthreads();
    for (int q = tid; q < ne * LOC; q += NT) {
      const int g = q / LOC, u = q - g * LOC;
      float s = 0.0f;
      for (int j = 0; j < N; ++j) s = s + L.D1[(size_t)(g * N + j) * H + u];
      L.DR2[g * H + u] = s;
    }
    grad_dw<WAVES>(part, N, HEAD, L.D1 + LOC, H, L.A2, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, HEAD, L.D1 + LOC, H, L.A2, H, L.D0, H, rows);
    __syncthreads();
    grad_dw<WAVES>(part, N, ADULT2, L.D0, H, L.A1, H, rows, L.LIVE_ROW, 1, first, 0);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, ADULT2, L.D0, H, L.A1, H, L.D1, H, rows);
    grad_dw<WAVES>(part, N, ROBOT2, L.DR2, H, L.R1, H, ne, L.LIVE, 1, first, 3);
    grad_dx<GRAD_DX_RELU, WAVES>(P, N, ROBOT2, L.DR2, H, L.R1, H, L.DR1, H, ne);
    __syncthreads();
    grad_dw<WAVES>(part, N, ADULT0, L.D1, H, L.X, KX, rows, L.LIVE_ROW, 1, first, 0);
    grad_dw<WAVES>(part, N, ROBOT0, L.DR1, H, L.RIN, 4, ne, L.LIVE, 1, first, WAVES - 1);
  }
}

__global__ __launch_bounds__(64 * EBC_SAIL_GRAD_WAVES) void sail_grad_kernel(const float *__restrict__ P, const SailGradLaunch a) {
  extern __shared__ float4 sail_grad_lds4[];
  constexpr int C = EBC_SAIL_GRAD_CHUNK;
  const int N = a.N, G = ebc_sail::grad_group_envs(N);
  double *const loss = reinterpret_cast<double *>(sail_grad_lds4);  // thread 0's, with the count behind it
  long long *const count = reinterpret_cast<long long *>(sail_grad_lds4) + 1;
  if (threadIdx.x == 0) {
    *loss = 0.0;
    *count = 0;
  }
  const long long c0 = ((long long)a.chunk0 + blockIdx.x) * C;
  const int nc = a.E - c0 < C ? (int)(a.E - c0) : C;  // envs of this chunk, >= 1
  float *const part = a.partial + (size_t)blockIdx.x * ebc_sail::packed_floats(N);
  for (int g0 = 0; g0 < nc; g0 += G) sail_grad_group(P, a, part, c0 + g0, nc - g0 < G ? nc - g0 : G, g0 == 0);
  if (threadIdx.x == 0) {
    a.loss_part[blockIdx.x] = *loss;
    a.count_part[blockIdx.x] = *count;
  }
}

}  // namespace ebc
