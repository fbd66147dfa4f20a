// ebc_sarl_grad_layers.h — the LAYER form of the SARL gradient (ebc_sarl_grad_rule.h): the same rule, the same bytes, layer
// by layer over a whole run of states on the float32 matrix instruction, activations and deltas in device memory.  No LDS
// limit on R and hidden layers up to EBC_SARL_GRAD_LAYERS_MAX_WIDTH; the chunk form (ebc_sarl_grad.h) is untouched.
//
// Why the bytes are the rule's.  v_mfma_f32_32x32x2_f32 is, per output, a k-ordered float32 fmaf chain: one rounding per
// product, no wider accumulation, C/D never flushed.  All three chains of the rule are such chains: the forward (k over a
// layer's inputs ascending from 0, the bias added after the chain), dx (u over the layer's units ascending from 0) and dW (over a
// chunk's live states and their rows ascending from 0; the bias row is the same chain with x = 1: fmaf(d, 1, acc) is acc + d).
// A tile never splits a chain, so which lane owns which output changes no byte.
//
// What must enter nothing (rows at or past n, states that are not live, the pad of an odd chain, a tile's edge) enters as
// the identity term (+0) * (-0): BOTH operands are replaced (either may be NaN), and adding -0 changes no accumulator, not
// even -0, which fmaf(+0, +0, -0) would turn into +0.  The forward and dx kernels mask only the chain's pad: a dead row's
// garbage stays in that row, and every reader of rows (the glue kernels by n, dW by the slot flags) leaves it out.
//
// dW: a workgroup owns a 32 x 32 tile of a layer's [K + 1][Op] block and walks the run's chunks ascending: a chunk's chain
// starts at +0 (one wave runs it whole), its result is added to the tile's float64 sums (registers), which start from 0 or
// from the run before (acc64) and leave rounded once (grad) after the last run.  No partials in memory, no atomics, nothing
// that depends on timing or on the grid.
//
// Fragment maps of the 32x32x2 instruction (lane l, i = l & 31, h = l >> 5): A[i][k = h], B[k = h][j = i], and register v
// of the result is row 8 (v >> 2) + 4 h + (v & 3), column i.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_cadrl_grad_rule.h"
#include "ebc_sarl_grad_rule.h"

namespace ebc {

typedef float layers_f32x16 __attribute__((ext_vector_type(16)));

#define EBC_LAYERS_AHEAD 4  // steps of a chain whose operands are loaded before the first of their instructions runs
#define EBC_LAYERS_ZERO16 {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}

// n, live and the slot flags of a run: a thread per row slot q = b * R + r of the run's states b0 .. b0 + Bp
__global__ __launch_bounds__(256) void layers_rows(const long long *__restrict__ n_valid, const unsigned char *__restrict__ mask, long long b0,
                                                   int Bp, int R, int *N, int *LIVE, int *SLOT) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)Bp * R) return;
  const int b = (int)(q / R), r = (int)(q - (long long)b * R);
  const int n = ebc_cadrl::clamp_rows(n_valid ? n_valid[b0 + b] : (long long)R, R);
  const bool live = ebc_cadrl::grad_live(!mask || mask[b0 + b] != 0, n);
  SLOT[q] = live && r < n ? 1 : 0;
  if (r == 0) N[b] = n, LIVE[b] = live ? 1 : 0;
}

// Y[q][u] = [relu](chain over k of X[q][k] * W[k][u] from 0, + bias[u]) for the Q rows q and the O units of a layer
// W[k][Op] | bias[Op] with K1 + K2 inputs: the first K1 from X1[q][.], the other K2 (attention's layer 0: the mean) from
// X2[q / R][.], as ONE chain.  A wave owns 32 rows x 64 units (two accumulators); a workgroup is four such row tiles.
// Whole pairs of inputs from one source run without a condition in the loop (a lane past the layer's units reads its last
// unit's weights and stores nothing), so the loads of several steps are in flight together; the pair that straddles the
// two sources and an odd chain's last term go through `single`, which gives the pad the identity term.
template <bool RELU>
__global__ __launch_bounds__(256) void layers_forward(const float *__restrict__ W, int K1, int K2, int O, int Op, const float *__restrict__ X1,
                                                      int s1, const float *__restrict__ X2, int s2, int R, float *__restrict__ Y, int ys,
                                                      long long Q) {
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const long long q0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (q0 >= Q) return;
  const int u0 = blockIdx.y * 64, K = K1 + K2;
  const long long q = q0 + i < Q ? q0 + i : Q - 1;  // rows past the end: the last one, not stored
  const float *x1 = X1 + q * s1, *x2 = K2 ? X2 + (q / R) * s2 : X1;
  const int ua = u0 + i, ub = u0 + 32 + i;
  const float *wa = W + (ua < O ? ua : O - 1), *wb = W + (ub < O ? ub : O - 1);
  layers_f32x16 acc0 = EBC_LAYERS_ZERO16, acc1 = EBC_LAYERS_ZERO16;
  const auto pairs = [&](const float *x, int k, int n) {  // n whole pairs: inputs k, k + 1, ... of the layer from x[0], x[1], ...
    const float *xp = x + h, *pa = wa + (size_t)(k + h) * Op, *pb = wb + (size_t)(k + h) * Op;
    int p = 0;
    for (; p + EBC_LAYERS_AHEAD <= n; p += EBC_LAYERS_AHEAD) {  // the loads of EBC_LAYERS_AHEAD steps, then their instructions
      float a[EBC_LAYERS_AHEAD], b0[EBC_LAYERS_AHEAD], b1[EBC_LAYERS_AHEAD];
#pragma unroll
      for (int j = 0; j < EBC_LAYERS_AHEAD; ++j)
        a[j] = xp[2 * (p + j)], b0[j] = pa[(size_t)2 * (p + j) * Op], b1[j] = pb[(size_t)2 * (p + j) * Op];
#pragma unroll
      for (int j = 0; j < EBC_LAYERS_AHEAD; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b0[j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b1[j], acc1, 0, 0, 0);
      }
    }
    for (; p < n; ++p) {
      const float a = xp[2 * p], b0 = pa[(size_t)2 * p * Op], b1 = pb[(size_t)2 * p * Op];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
  };
  const auto single = [&](int k0) {
    const int k = k0 + h;
    const bool in = k < K;
    const float a = in ? (k < K1 ? x1[k] : x2[k - K1]) : 0.0f;
    const float b0 = in ? wa[(size_t)k * Op] : -0.0f, b1 = in ? wb[(size_t)k * Op] : -0.0f;
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
  };
  int k0 = K1 / 2 * 2;
  pairs(x1, 0, K1 / 2);
  if (k0 < K1) single(k0), k0 += 2;
  if (k0 < K) {
    const int n = (K - k0) / 2;
    pairs(x2 + (k0 - K1), k0, n);
    k0 += 2 * n;
    if (k0 < K) single(k0);
  }
  const float *bias = W + (size_t)K * Op;
  const float ba = ua < O ? bias[ua] : 0.0f, bb = ub < O ? bias[ub] : 0.0f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const long long qq = q0 + 8 * (v >> 2) + 4 * h + (v & 3);
    if (qq >= Q) continue;
    if (ua < O) {
      const float y = acc0[v] + ba;
      Y[qq * ys + ua] = RELU ? ebc_cadrl::grad_relu(y) : y;
    }
    if (ub < O) {
      const float y = acc1[v] + bb;
      Y[qq * ys + ub] = RELU ? ebc_cadrl::grad_relu(y) : y;
    }
  }
}

// out[q][k] = (RELU: relu_back(act[q][k], dx) else dx), dx the chain over the layer's units u ascending of
// W[k][u] * delta[q][u] from 0, for the Q rows and the layer's K inputs.  act may be out (the activation's delta takes its
// place).  A wave owns 32 rows x 64 inputs; whole pairs of units without a condition, an odd last unit with the identity pad.
template <bool RELU>
__global__ __launch_bounds__(256) void layers_dx(const float *__restrict__ W, int K, int O, int Op, const float *__restrict__ delta, int ds,
                                                 const float *act, int as, float *out, int os, long long Q) {
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const long long q0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (q0 >= Q) return;
  const int k0 = blockIdx.y * 64;
  const long long q = q0 + i < Q ? q0 + i : Q - 1;
  const float *d = delta + q * ds + h;
  const int ka = k0 + i, kb = k0 + 32 + i;
  const float *wa = W + (size_t)(ka < K ? ka : K - 1) * Op + h, *wb = W + (size_t)(kb < K ? kb : K - 1) * Op + h;
  layers_f32x16 acc0 = EBC_LAYERS_ZERO16, acc1 = EBC_LAYERS_ZERO16;
  const int n = O / 2;
  int p = 0;
  for (; p + EBC_LAYERS_AHEAD <= n; p += EBC_LAYERS_AHEAD) {
    float a[EBC_LAYERS_AHEAD], b0[EBC_LAYERS_AHEAD], b1[EBC_LAYERS_AHEAD];
#pragma unroll
    for (int j = 0; j < EBC_LAYERS_AHEAD; ++j) a[j] = d[2 * (p + j)], b0[j] = wa[2 * (p + j)], b1[j] = wb[2 * (p + j)];
#pragma unroll
    for (int j = 0; j < EBC_LAYERS_AHEAD; ++j) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b0[j], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b1[j], acc1, 0, 0, 0);
    }
  }
  for (; p < n; ++p) {
    const float a = d[2 * p], b0 = wa[2 * p], b1 = wb[2 * p];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
  }
  if (2 * n < O) {  // the odd last unit on the lower half, the pad on the upper
    const float a = h ? 0.0f : d[2 * n], b0 = h ? -0.0f : wa[2 * n], b1 = h ? -0.0f : wb[2 * n];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const long long qq = q0 + 8 * (v >> 2) + 4 * h + (v & 3);
    if (qq >= Q) continue;
    if (ka < K) out[qq * os + ka] = RELU ? ebc_cadrl::grad_relu_back(act[qq * as + ka], acc0[v]) : acc0[v];
    if (kb < K) out[qq * os + kb] = RELU ? ebc_cadrl::grad_relu_back(act[qq * as + kb], acc1[v]) : acc1[v];
  }
}

// A layer's dW and db over a run.  The layer's block is [K1 + K2 + 1][Op] (the last row the bias); the chain of entry
// (k, u) runs over the slots q < Q ascending whose flag is set, chunk by chunk (cs slots a chunk, cs even), from +0 in every
// chunk: fmaf(delta[q][u], x[q][k], .), x from X1[q][k], from X2[q][k - K1] or 1 (the bias row).  The chunks' results are
// added ascending in float64: from 0 when `first`, else from acc64; after the run into grad, rounded once and canonical,
// when `last`, else back into acc64.  Pad entries (u >= O) get 0.
// A workgroup of EBC_LAYERS_DW_WAVES waves owns one 32 x 32 tile.  In a round every wave runs the chains of its own two
// consecutive chunks (two accumulators) and leaves the two results in LDS; then every thread adds, for its two entries of the
// tile, the round's results in chunk order to its float64 sums.  Which wave ran a chunk changes nothing: a chunk's chain is
// whole, and the float64 sum walks the chunks ascending.  Both operands of a term are loaded whatever the flag says (a slot
// past the end reads the last one) and selected afterwards, so the loads do not wait for the flags.
#define EBC_LAYERS_DW_WAVES 8
__global__ __launch_bounds__(64 * EBC_LAYERS_DW_WAVES) void layers_dw(const float *__restrict__ X1, int s1, int K1, const float *__restrict__ X2,
                                                                      int s2, int K2, const float *__restrict__ delta, int ds, int O, int Op,
                                                                      const int *__restrict__ flag, long long Q, int cs, int first, int last,
                                                                      double *acc64, float *grad) {
  constexpr int NW = EBC_LAYERS_DW_WAVES, NT = 64 * NW;
  __shared__ float part[NW * 2 * 1024];  // [wave][chunk of the pair][register v][lane]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int K = K1 + K2, k = blockIdx.x * 32 + i, u = blockIdx.y * 32 + i;
  // the entries (two of the tile's 1024) whose float64 sums this thread keeps: entry e is register e >> 6 of lane e & 63
  size_t at[2];
  bool mine[2], pad[2];
  double sum[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = tid + NT * j, v = e >> 6, ln = e & 63;
    const int kk = blockIdx.x * 32 + 8 * (v >> 2) + 4 * (ln >> 5) + (v & 3), uu = blockIdx.y * 32 + (ln & 31);
    mine[j] = kk <= K && uu < Op, pad[j] = uu >= O, at[j] = (size_t)kk * Op + uu;
    sum[j] = first || !mine[j] ? 0.0 : acc64[at[j]];
  }
  // this lane's operands: x[q][k] at xs[q * xstride] (a row past the block reads the first input and is not stored)
  const float *xs = k < K1 ? X1 + k : k < K ? X2 + (k - K1) : X1;
  const long long xstride = k >= K1 && k < K ? s2 : s1;
  const float *dl = delta + (u < O ? u : O - 1);
  const bool xin = k < K, xone = k == K, uin = u < O;
  const auto term = [&](long long q, long long qend, float &a, float &b) {
    const long long qq = q < Q ? q : Q - 1;
    const float x = xs[qq * xstride], d = dl[qq * ds];
    const bool on = q < qend && flag[qq] != 0;
    a = on ? (xin ? x : xone ? 1.0f : 0.0f) : 0.0f;
    b = on && uin ? d : -0.0f;
  };
  const long long chunks = (Q + cs - 1) / cs;
  for (long long c0 = 0; c0 < chunks; c0 += 2 * NW) {
    const long long ca = c0 + 2 * wave;
    if (ca < chunks) {
      const long long qa = ca * cs, qa_end = qa + cs < Q ? qa + cs : Q;
      const long long qb = qa_end, qb_end = qb + cs < Q ? qb + cs : Q;  // empty when ca + 1 == chunks
      layers_f32x16 acc0 = EBC_LAYERS_ZERO16, acc1 = EBC_LAYERS_ZERO16;
      int t = 0;
      for (; t + 2 * EBC_LAYERS_AHEAD <= cs; t += 2 * EBC_LAYERS_AHEAD) {
        float a0[EBC_LAYERS_AHEAD], b0[EBC_LAYERS_AHEAD], a1[EBC_LAYERS_AHEAD], b1[EBC_LAYERS_AHEAD];
#pragma unroll
        for (int j = 0; j < EBC_LAYERS_AHEAD; ++j) {
          term(qa + t + 2 * j + h, qa_end, a0[j], b0[j]);
          term(qb + t + 2 * j + h, qb_end, a1[j], b1[j]);
        }
#pragma unroll
        for (int j = 0; j < EBC_LAYERS_AHEAD; ++j) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc1, 0, 0, 0);
        }
      }
      for (; t < cs; t += 2) {
        float a0, b0, a1, b1;
        term(qa + t + h, qa_end, a0, b0);
        term(qb + t + h, qb_end, a1, b1);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc1, 0, 0, 0);
      }
      float *mp = part + (size_t)wave * 2048 + lane;
#pragma unroll
      for (int v = 0; v < 16; ++v) mp[v * 64] = acc0[v], mp[1024 + v * 64] = acc1[v];
    }
    __syncthreads();
    const int here = chunks - c0 < 2 * NW ? (int)(chunks - c0) : 2 * NW;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      for (int c = 0; c < here; ++c) sum[j] = sum[j] + (double)part[c * 1024 + tid + NT * j];
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!mine[j]) continue;
    if (last) grad[at[j]] = pad[j] ? 0.0f : ebc_cadrl::canon((float)sum[j]);
    else acc64[at[j]] = sum[j];
  }
}

// g[b][k] = over_rows(0 + h1[b][0][k] + h1[b][1][k] + ..., n): a thread per (state, k); G[b] holds it for the forward, and
// GQ[q] a copy per row slot of the state for layer 4's dW, whose operands are indexed by the slot
__global__ __launch_bounds__(256) void layers_mean(const float *__restrict__ H1, int hs, int H, int R, const int *__restrict__ N, int Bp, float *G,
                                                   float *GQ, int gs) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Bp * H) return;
  const int b = (int)(idx / H), k = (int)(idx - (long long)b * H), n = N[b];
  if (n < 1) return;
  float acc = 0.0f;
  for (int r = 0; r < n; ++r) acc = acc + H1[((size_t)b * R + r) * hs + k];
  const float g = ebc_sarl::over_rows(acc, n);
  G[(size_t)b * gs + k] = g;
  for (int r = 0; r < R; ++r) GQ[((size_t)b * R + r) * gs + k] = g;
}

// The softmax over a state's scores, the weighted sum of its features and the joint vector: a workgroup of 128 threads per
// state.  SC [Q] scores -> WT [Q] weights, attention (when given), J[b] = cat(x[b][0][0 .. S), wf).
__global__ __launch_bounds__(128) void layers_softmax(const float *__restrict__ SC, const float *__restrict__ FT, int fs, int F,
                                                      const float *__restrict__ rows, int T, int S, int R, const int *__restrict__ N, float *WT,
                                                      float *attention, float *J, int js) {
  __shared__ float e[EBC_SARL_GRAD_LAYERS_MAX_ROWS];
  const int b = blockIdx.x, tid = threadIdx.x, n = N[b];
  const size_t q0 = (size_t)b * R;
  if (tid < n) e[tid] = ebc_sarl::score_exp(SC[q0 + tid]);
  __syncthreads();
  float sum = 0.0f;
  for (int r = 0; r < n; ++r) sum = sum + e[r];
  __syncthreads();
  if (tid < R) {
    float w = 0.0f;
    if (tid < n) {
      w = ebc_sarl::quotient(e[tid], sum);
      e[tid] = w;
      WT[q0 + tid] = w;
    }
    if (attention) attention[q0 + tid] = tid < n ? ebc_cadrl::canon(w) : 0.0f;
  }
  __syncthreads();
  if (n < 1) return;
  for (int k = tid; k < S; k += 128) J[(size_t)b * js + k] = rows[q0 * T + k];
  for (int f = tid; f < F; f += 128) {
    float acc = 0.0f;
    for (int r = 0; r < n; ++r) acc = ebc_cadrl::chain(e[r], FT[(q0 + r) * fs + f], acc);
    J[(size_t)b * js + S + f] = acc;
  }
}

// value, live, loss and seed of the run's states: a thread per state
__global__ __launch_bounds__(256) void layers_seed(const float *__restrict__ OUT, const int *__restrict__ N, const int *__restrict__ LIVE,
                                                   const float *__restrict__ target, long long b0, int Bp, float grad_scale, float *value,
                                                   double *LOSS, float *SEED) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= Bp) return;
  const int n = N[b];
  const float val = ebc_cadrl::grad_value(n >= 1 ? OUT[b] : 0.0f, n);
  if (value) value[b0 + b] = val;
  double loss = 0.0;
  float seed = 0.0f;
  if (LIVE[b]) {
    const float d = ebc_cadrl::grad_diff(val, target[b0 + b]);
    loss = ebc_cadrl::grad_loss(d);
    seed = grad_scale * d;
  }
  LOSS[b] = loss;
  SEED[b] = seed;
}

// The run's loss and count: per chunk of `chunk` states the float64 sum of the live states' losses in state order from 0,
// the chunks added ascending; continues acc64[0] / acc64[1] of the run before unless `first`; `last`: out as the rule's.
// One wave: 64 chunks' sums at a time, a lane each, then added in chunk order.
__global__ __launch_bounds__(64) void layers_loss(const double *__restrict__ LOSS, const int *__restrict__ LIVE, int Bp, int chunk, int first,
                                                  int last, double *acc64, double *loss_sum, long long *count) {
  const int lane = threadIdx.x;
  double total = first ? 0.0 : acc64[0];
  long long live = first ? 0 : reinterpret_cast<long long *>(acc64)[1];
  const int chunks = (Bp + chunk - 1) / chunk;
  for (int c0 = 0; c0 < chunks; c0 += 64) {
    double mine = 0.0;
    int cnt = 0;
    const int c = c0 + lane;
    if (c < chunks)
      for (int s = c * chunk; s < (c + 1) * chunk && s < Bp; ++s)
        if (LIVE[s]) mine = mine + LOSS[s], cnt += 1;
    const int m = chunks - c0 < 64 ? chunks - c0 : 64;
    for (int j = 0; j < m; ++j) {
      total = total + __shfl(mine, j);
      live += __shfl(cnt, j);
    }
  }
  if (lane != 0) return;
  if (last) {
    *loss_sum = ebc_cadrl::canon(total);
    *count = live;
  } else {
    acc64[0] = total;
    reinterpret_cast<long long *>(acc64)[1] = live;
  }
}

// softmax' and weighted' of a run's states: a workgroup of 128 threads per state with at least one row.  dwf = DJ[b][S ..];
// c[r] = chain over f of dwf[f] * centred(ft[r][f], wf[f]); m = chain over r of w[r] * c[r]; SC[q] = score_back(w, c, m)
// (the score's delta takes the score's place) and FT[q][f] = w[r] * dwf[f] (the features' delta takes theirs).
__global__ __launch_bounds__(128) void layers_softmax_back(const float *__restrict__ DJ, const float *__restrict__ J, int js, int S, int F, int R,
                                                           const int *__restrict__ N, const float *__restrict__ WT, float *SC, float *FT, int fs) {
  __shared__ float c[EBC_SARL_GRAD_LAYERS_MAX_ROWS], w[EBC_SARL_GRAD_LAYERS_MAX_ROWS];
  const int b = blockIdx.x, tid = threadIdx.x, n = N[b];
  if (n < 1) return;
  const size_t q0 = (size_t)b * R;
  const float *dwf = DJ + (size_t)b * js + S, *wf = J + (size_t)b * js + S;
  if (tid < n) {
    float acc = 0.0f;
    for (int f = 0; f < F; ++f) acc = ebc_cadrl::chain(dwf[f], ebc_sarl::centred(FT[(q0 + tid) * fs + f], wf[f]), acc);
    c[tid] = acc;
    w[tid] = WT[q0 + tid];
  }
  __syncthreads();
  float m = 0.0f;
  for (int r = 0; r < n; ++r) m = ebc_cadrl::chain(w[r], c[r], m);
  if (tid < n) SC[q0 + tid] = ebc_sarl::score_back(w[tid], c[tid], m);
  for (int idx = tid; idx < n * F; idx += 128) {
    const int r = idx / F, f = idx - r * F;
    FT[(q0 + r) * fs + f] = w[r] * dwf[f];
  }
}

// mean' and h1': a thread per (state, k).  D2 = dx of mlp2's layer 0, D4 = dx of attention's layer 0 ([H | H] inputs with
// global state); dm = over_rows(0 + D4[r][H + k] ..., n); H1[q][k] = h1_back(h1, D2, D4[.][k], dm): h1's delta takes its place.
__global__ __launch_bounds__(256) void layers_h1_back(const float *__restrict__ D2, int d2s, const float *__restrict__ D4, int d4s, int H, int R,
                                                      int global, const int *__restrict__ N, int Bp, float *H1, int hs) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Bp * H) return;
  const int b = (int)(idx / H), k = (int)(idx - (long long)b * H), n = N[b];
  if (n < 1) return;
  const size_t q0 = (size_t)b * R;
  float dm = 0.0f;
  if (global) {
    float dg = 0.0f;
    for (int r = 0; r < n; ++r) dg = dg + D4[(q0 + r) * d4s + H + k];
    dm = ebc_sarl::over_rows(dg, n);
  }
  for (int r = 0; r < n; ++r) {
    float *o = H1 + (q0 + r) * hs + k;
    *o = ebc_sarl::h1_back(*o, D2[(q0 + r) * d2s + k], D4[(q0 + r) * d4s + k], dm, global);
  }
}

// a batch without states: zero gradient, loss 0, count 0
__global__ __launch_bounds__(256) void layers_empty(size_t PF, float *grad, double *loss_sum, long long *count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < PF) grad[i] = 0.0f;
  if (i == 0) *loss_sum = 0.0, *count = 0;
}

}  // namespace ebc
