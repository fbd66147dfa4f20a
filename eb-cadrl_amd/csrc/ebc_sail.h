// ebc_sail.h — the SAIL network (rl/policy/sail.py:9-101) and the decision around it (sail.py:114-156) as ONE kernel:
// from the env's float64 robot state and observation rows to action[E][2], float32, the arithmetic of ebc_sail_rule.h.
//
// The network itself is sail_group below, a device function for a group of envs on the waves of a workgroup with its
// inputs behind accessors: sail_kernel (this header, eight waves, inputs in global memory) and the rollout kernel of
// ebc_step_k with EBC_ROBOT_SAIL (ebc_rollout.h, four waves, inputs in its LDS state) both call it.
//
// A workgroup of eight waves owns G = group_envs(N) whole envs (G * N <= 48 adult rows, or one env), so the softmax over an
// env's N rows and the crowd sum are workgroup-local.  Every layer is at most 64 units wide and a wave has 64 lanes: lane
// u owns unit u.  A wave carries EBC_SAIL_T rows at once: a k step loads ONE weight W[k][u] (64 adjacent floats, coalesced;
// the packed image is about 190 KB and stays in L2) and spends it on T fmaf against x_t[k], which every lane reads from
// the same LDS address (a broadcast; four k steps at a time as one 16-byte read).  The k order of a unit's chain is the
// header's, so the result is the host build's byte for byte and does not depend on T, on the tile a row falls in or on
// the env's place in the batch.  Activations stay in LDS from the casts to the planner; nothing intermediate is written
// to memory.  No atomics, no polling.
//
// T, the waves and G are what measured best at 4096 envs x 5 adults (profiles/sail_decision.txt): the kernel is bound by
// the latency of its barrier-separated layers, not by the weights' traffic, so tiles that spread evenly over the waves
// (40 rows = 8 tiles of 5 on 8 waves) beat larger tiles (T = 8 on 4 waves: 0.082 ms against 0.052 ms).
//
// LDS, in floats (rows = G * N, KX = max(4 N, 64)): X [rows][KX] the transformed frame, later feat_pairwise [rows][64];
// A, B [rows][64] the ping-pong of the row layers; per env: E1, E2 [G][64], E3 [G][128] (feat_task | feat_crowd), the
// robot and task inputs [G][4] each, the frame [rows][4]; the logits and the scores [rows] each.  48 KB of rows at the most.
//
// Rows at or past N of an env are never read.  An env whose row count is not N is computed like any other (its first N
// rows are inside the buffer) and its outputs are replaced by selection.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_sail_rule.h"

#ifndef EBC_SAIL_T
#define EBC_SAIL_T 5      // rows a wave carries at once
#endif
#ifndef EBC_SAIL_WAVES
#define EBC_SAIL_WAVES 8  // waves per workgroup
#endif

namespace ebc {

struct SailLaunch {
  const double *robot;        // [E][9]
  const double *ob;           // [E][R][5]
  const long long *n_rows;    // [E] or nullptr = N
  double *action;             // [E][2]
  float *feat_joint;          // [E][64] or nullptr
  int E, R, N;
};

// floats of the LDS arrays of a group of G envs (sail_lds below)
__host__ __device__ inline size_t sail_lds_floats(int G, int N) {
  const int rows = G * N, KX = 4 * N > 64 ? 4 * N : 64;
  return (size_t)rows * (KX + 64 + 64 + 4 + 2) + (size_t)G * (64 + 64 + 128 + 4 + 4) + 8;
}
inline size_t sail_lds_floats(int N) { return sail_lds_floats(ebc_sail::group_envs(N), N); }

// y[r][yoff + u] = (relu of) layer(x[r][0 .. K)) for r < nrows, u < O: tiles of T rows dealt to the WAVES waves from `first`
template <bool RELU, int WAVES>
__device__ __forceinline__ void sail_layer(const float *__restrict__ P, int N, int l, const float *x, int xs, float *y, int ys, int yoff,
                                           int nrows, int first) {
  constexpr int T = EBC_SAIL_T, H = EBC_SAIL_HIDDEN;
  const int lane = threadIdx.x & 63, wave = ((threadIdx.x >> 6) - first + WAVES) % WAVES;
  const int K = ebc_sail::layer_in(l, N), O = ebc_sail::layer_out(l);
  const float *W = P + ebc_sail::layer_offset(l, N) + lane;
  const float bias = W[(size_t)K * H];
  for (int r0 = wave * T; r0 < nrows; r0 += WAVES * T) {
    float acc[T];
    const float4 *xr[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      acc[t] = bias;
      const int r = r0 + t < nrows ? r0 + t : nrows - 1;  // a tile's rows past the end read the last row and store nothing
      xr[t] = reinterpret_cast<const float4 *>(x + (size_t)r * xs);
    }
#pragma unroll 2
    for (int k4 = 0; k4 < K / 4; ++k4) {  // every K is a multiple of 4
      const float w0 = W[(size_t)(4 * k4) * H], w1 = W[(size_t)(4 * k4 + 1) * H], w2 = W[(size_t)(4 * k4 + 2) * H],
                  w3 = W[(size_t)(4 * k4 + 3) * H];
      float4 v[T];
#pragma unroll
      for (int t = 0; t < T; ++t) v[t] = xr[t][k4];
      float xk[T];
#pragma unroll
      for (int t = 0; t < T; ++t) xk[t] = v[t].x;
      ebc_sail::unit_step<T>(acc, w0, xk);
#pragma unroll
      for (int t = 0; t < T; ++t) xk[t] = v[t].y;
      ebc_sail::unit_step<T>(acc, w1, xk);
#pragma unroll
      for (int t = 0; t < T; ++t) xk[t] = v[t].z;
      ebc_sail::unit_step<T>(acc, w2, xk);
#pragma unroll
      for (int t = 0; t < T; ++t) xk[t] = v[t].w;
      ebc_sail::unit_step<T>(acc, w3, xk);
    }
    if (lane < O) {
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (r0 + t < nrows) y[(size_t)(r0 + t) * ys + yoff + lane] = RELU ? ebc_sail::relu(acc[t]) : acc[t];
    }
  }
}

// The LDS arrays of one group of G envs of N adults (every array starts at a multiple of 4 floats); `planned` and
// `feat_joint` are where sail_group leaves an env's results: planned[g * 64 + c], feat_joint[g * 64 + u].
struct SailLds {
  float *X, *A, *B, *E1, *E2, *E3, *RIN, *TIN, *FR, *LG, *SC;
  int KX;
  __device__ __forceinline__ const float *planned() const { return E2; }
  __device__ __forceinline__ const float *feat_joint() const { return E1; }
};
__device__ __forceinline__ SailLds sail_lds(float *base, int G, int N) {
  constexpr int H = EBC_SAIL_HIDDEN;
  const int rows_max = G * N;
  SailLds L;
  L.KX = 4 * N > 64 ? 4 * N : 64;
  L.X = base;
  L.A = L.X + (size_t)rows_max * L.KX;
  L.B = L.A + (size_t)rows_max * H;
  L.E1 = L.B + (size_t)rows_max * H;
  L.E2 = L.E1 + G * H;
  L.E3 = L.E2 + G * H;
  L.RIN = L.E3 + G * 2 * H;
  L.TIN = L.RIN + G * 4;
  L.FR = L.TIN + G * 4;
  L.LG = L.FR + (size_t)rows_max * 4;
  L.SC = L.LG + rows_max;
  return L;
}

// Inputs of sail_group from global memory: robot [E][9], ob [E][R][5], the group's first env e0.
struct SailGlobalSrc {
  const double *robot_base, *ob;
  int R;
  long long e0;
  __device__ __forceinline__ const double *robot(int g) const { return robot_base + (size_t)(e0 + g) * 9; }
  __device__ __forceinline__ float frame(int g, int i, int c) const { return (float)ob[((size_t)(e0 + g) * R + i) * 5 + c]; }
};

// The network for `ne` <= G envs of N adults on the WAVES waves of a workgroup (all 64 * WAVES threads call it; it
// holds workgroup barriers): from src.robot(g) (9 doubles of env g) and src.frame(g, i, c) (element c < 4 of row
// i < N, cast to float32) to L.planned() and L.feat_joint(), readable by every thread when it returns.  Where the
// inputs live (global memory for sail_kernel, the rollout kernel's LDS state) and how many waves share the rows do not
// touch a unit's chain, so the results are ebc_sail_rule.h's whatever WAVES and G are.
template <int WAVES, typename Src>
__device__ __forceinline__ void sail_group(const float *__restrict__ P, int N, const SailLds &L, int ne, const Src &src) {
  constexpr int H = EBC_SAIL_HIDDEN, LOC = EBC_SAIL_LOCAL, NT = 64 * WAVES;
  using namespace ebc_sail;
  const int KX = L.KX, tid = threadIdx.x, rows = ne * N;  // adult rows this call has
  float *const X = L.X, *const A = L.A, *const B = L.B, *const E1 = L.E1, *const E2 = L.E2, *const E3 = L.E3;
  float *const RIN = L.RIN, *const TIN = L.TIN, *const FR = L.FR, *const LG = L.LG, *const SC = L.SC;

  // the casts
  for (int g = tid; g < ne; g += NT) {
    float rv[6], task[4];
    robot_vectors(src.robot(g), rv, task);
    for (int c = 0; c < 4; ++c) {
      RIN[4 * g + c] = rv[c];
      TIN[4 * g + c] = task[c];
    }
  }
  for (int q = tid; q < rows * 4; q += NT) {
    const int r = q >> 2, c = q & 3, g = r / N, i = r - g * N;
    FR[q] = src.frame(g, i, c);
  }
  __syncthreads();
  for (int q = tid; q < rows * 4 * N; q += NT) {
    const int r = q / (4 * N), k = q - r * 4 * N, g = r / N, i = r - g * N;
    X[(size_t)r * KX + k] = frame_input(FR + (size_t)g * N * 4, i, k);
  }
  __syncthreads();
  sail_layer<true, WAVES>(P, N, ADULT0, X, KX, A, H, 0, rows, 0);
  sail_layer<true, WAVES>(P, N, ROBOT0, RIN, 4, E1, H, 0, ne, WAVES - 1);
  __syncthreads();
  sail_layer<true, WAVES>(P, N, ADULT2, A, H, B, H, 0, rows, 0);
  sail_layer<true, WAVES>(P, N, ROBOT2, E1, H, E2, H, 0, ne, WAVES - 1);
  __syncthreads();
  // emb_concat = [emb_robot | emb_adult] per row in A
  sail_layer<true, WAVES>(P, N, HEAD, B, H, A, H, LOC, rows, 0);
  for (int q = tid; q < rows * LOC; q += NT) {
    const int r = q / LOC, u = q - r * LOC;
    A[(size_t)r * H + u] = E2[(r / N) * H + u];
  }
  sail_layer<true, WAVES>(P, N, TASK0, TIN, 4, E1, H, 0, ne, WAVES - 1);
  __syncthreads();
  sail_layer<true, WAVES>(P, N, EMBED, A, H, B, H, 0, rows, 0);
  sail_layer<true, WAVES>(P, N, TASK2, E1, H, E3, 2 * H, 0, ne, WAVES - 1);
  __syncthreads();
  sail_layer<true, WAVES>(P, N, PAIR0, B, H, A, H, 0, rows, 0);
  __syncthreads();
  sail_layer<false, WAVES>(P, N, PAIR2, A, H, X, H, 0, rows, 0);  // feat_pairwise over the dead frame rows
  __syncthreads();
  sail_layer<true, WAVES>(P, N, ATT0, B, H, A, H, 0, rows, 0);
  __syncthreads();
  sail_layer<false, WAVES>(P, N, ATT2, A, H, LG, 1, 0, rows, 0);
  __syncthreads();
  // softmax over an env's logits (every lane of the env's wave, the same values) and the crowd sum, unit per lane
  {
    const int lane = tid & 63;
    for (int g = tid >> 6; g < ne; g += WAVES) {
      float *score = SC + g * N;  // every lane writes the same values
      softmax(LG + g * N, 1, N, score);
      float acc = 0.0f;
      for (int j = 0; j < N; ++j) acc = fmaf(X[(size_t)(g * N + j) * H + lane], score[j], acc);
      E3[g * 2 * H + H + lane] = acc;
    }
  }
  __syncthreads();
  sail_layer<true, WAVES>(P, N, JOINT, E3, 2 * H, E1, H, 0, ne, 0);
  __syncthreads();
  sail_layer<false, WAVES>(P, N, PLANNER, E1, H, E2, H, 0, ne, 0);
  __syncthreads();
}

// The stand-alone kernel (ebc_sail_forward): defined in the one unit that launches it, ebcsim_sail.hip; ebc_rollout.h
// includes this header for sail_group alone.
#ifdef EBC_SAIL_KERNEL
__global__ __launch_bounds__(64 * EBC_SAIL_WAVES) void sail_kernel(const float *__restrict__ P, const SailLaunch a) {
  extern __shared__ float4 sail_lds4[];
  constexpr int H = EBC_SAIL_HIDDEN, NT = 64 * EBC_SAIL_WAVES;
  using namespace ebc_sail;
  const int N = a.N, G = group_envs(N), tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * G;
  const int ne = a.E - e0 < G ? (int)(a.E - e0) : G;  // envs this workgroup has
  const SailLds L = sail_lds(reinterpret_cast<float *>(sail_lds4), G, N);
  const SailGlobalSrc src = {a.robot, a.ob, a.R, e0};
  sail_group<EBC_SAIL_WAVES>(P, N, L, ne, src);
  const float *E1 = L.feat_joint(), *E2 = L.planned();
  for (int q = tid; q < ne * 2; q += NT) {
    const int g = q >> 1, c = q & 1;
    const long long e = e0 + g;
    const bool rows_ok = !a.n_rows || a.n_rows[e] == (long long)N;
    a.action[(size_t)e * 2 + c] = action_of(E2[g * H + c], arrived(a.robot + (size_t)e * 9), rows_ok);
  }
  if (a.feat_joint) {
    for (int q = tid; q < ne * H; q += NT) {
      const int g = q / H;
      const long long e = e0 + g;
      const bool rows_ok = !a.n_rows || a.n_rows[e] == (long long)N;
      a.feat_joint[(size_t)e * H + (q - g * H)] = feature_of(E1[q], rows_ok);
    }
  }
}
#endif  // EBC_SAIL_KERNEL

}  // namespace ebc
