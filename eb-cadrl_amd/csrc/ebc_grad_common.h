// ebc_grad_common.h — what the gradient kernels share: the kernel that adds the chunks' partials (grad_reduce, every
// gradient unit's) and the row-slot layer forms and pass-loop blocks of the kernels whose states are R row slots side by
// side (ebc_sarl_grad.h, ebc_lstm_grad.h).  The scalar steps are ebc_cadrl_grad_rule.h's (chain, grad_relu, grad_relu_back,
// grad_value, grad_live, grad_diff, grad_loss, canon, clamp_rows), which the SARL and LSTM rules take over by `using`.
// CADRL's cadrl_layer / cadrl_dw / cadrl_dx (a wave per row tile, a separate `out`) and SAIL's forms are other mappings
// and stay in their headers.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_cadrl_grad_rule.h"

namespace ebc {

// out[q][u] for the slots q < nslots and every unit u of a layer W[k][Op] | bias[Op] with K1 + K2 inputs: the first K1 from
// in[q][.], the other K2 (SARL attention's layer 0: the mean) from in2[q / R][.]; grad_unit's chain, ReLU when asked.  A
// thread of the NT owns (a tile of 4 slots, unit u).  A literal K2 = 0 (in2 nullptr) folds the second loop away.
template <int NT, bool RELU>
__device__ __forceinline__ void grad_layer(const float *__restrict__ W, int K1, int K2, int O, int Op, const float *in, int is, const float *in2,
                                           int i2s, int R, float *out, int os, int nslots) {
  constexpr int TR = 4;
  const int tiles = (nslots + TR - 1) / TR;
  for (int idx = threadIdx.x; idx < tiles * O; idx += NT) {
    const int tile = idx / O, u = idx - tile * O, q0 = tile * TR;
    const float *xr[TR], *x2[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) {
      const int q = q0 + t < nslots ? q0 + t : nslots - 1;  // slots past the end: the last one, not stored
      xr[t] = in + (size_t)q * is;
      x2[t] = K2 ? in2 + (size_t)(q / R) * i2s : in;
    }
    float acc[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t] = 0.0f;
    for (int k = 0; k < K1; ++k) {
      const float w = W[(size_t)k * Op + u];
#pragma unroll
      for (int t = 0; t < TR; ++t) acc[t] = ebc_cadrl::chain(xr[t][k], w, acc[t]);
    }
    for (int k = 0; k < K2; ++k) {
      const float w = W[(size_t)(K1 + k) * Op + u];
#pragma unroll
      for (int t = 0; t < TR; ++t) acc[t] = ebc_cadrl::chain(x2[t][k], w, acc[t]);
    }
    const float b = W[(size_t)(K1 + K2) * Op + u];
#pragma unroll
    for (int t = 0; t < TR; ++t) {
      if (q0 + t >= nslots) continue;
      const float y = acc[t] + b;
      out[(size_t)(q0 + t) * os + u] = RELU ? ebc_cadrl::grad_relu(y) : y;
    }
  }
}

// a layer's dW and db into G (the layer's place in the chunk's partial, (K1 + K2 + 1) * Op floats) over the chunk's live
// states s < nc ascending and, with per_row, their rows r < N[s] ascending: delta at delta + q * ds, the input at x + q * xs
// (q the slot, or the state without per_row), inputs K1 .. of the state's x2 + s * x2s.  Pad entries get 0.  cont (a later
// pass of the chunk): the chain goes on from what this thread stored into G in the pass before, not from 0.
template <int NT>
__device__ __forceinline__ void grad_dw(float *__restrict__ G, int K1, int K2, int O, int Op, const float *delta, int ds, const float *x, int xs,
                                        const float *x2, int x2s, int R, int nc, const int *N, const int *live, bool per_row, bool cont) {
  const int K = K1 + K2, total = (K + 1) * Op;
  for (int idx = threadIdx.x; idx < total; idx += NT) {
    const int k = idx / Op, u = idx - k * Op;
    float acc = 0.0f;
    if (u < O) {
      if (cont) acc = G[idx];
      for (int s = 0; s < nc; ++s) {
        if (!live[s]) continue;
        const int n = per_row ? N[s] : 1, q0 = per_row ? s * R : s;
        if (k < K1) {
          for (int r = 0; r < n; ++r) acc = ebc_cadrl::chain(delta[(q0 + r) * ds + u], x[(q0 + r) * xs + k], acc);
        } else if (k < K) {
          const float xv = x2[s * x2s + (k - K1)];
          for (int r = 0; r < n; ++r) acc = ebc_cadrl::chain(delta[(q0 + r) * ds + u], xv, acc);
        } else {
          for (int r = 0; r < n; ++r) acc = acc + delta[(q0 + r) * ds + u];
        }
      }
    }
    G[idx] = acc;
  }
}

// the chain over a layer's units u ascending of w[u] * d[u] from 0; vec: both are 16-byte aligned
__device__ __forceinline__ float grad_dot(const float *__restrict__ w, const float *d, int O, bool vec) {
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
  return acc;
}

// act[q][k] = (RELU: relu_back(act[q][k], dx) else dx), dx the chain over the layer's units of W[k][u] * delta[q][u], for
// the inputs k0 <= k < k1 (stored at act[q][k - k0]) and the live slots (per_row: q = s * R + r, r < N[s]; else q = s)
template <int NT, bool RELU>
__device__ __forceinline__ void grad_dx(const float *__restrict__ W, int k0, int k1, int O, int Op, const float *delta, int ds, float *act, int as,
                                        int R, int nc, const int *N, const int *live, bool per_row, bool vec) {
  const int nq = per_row ? nc * R : nc;
  for (int idx = threadIdx.x; idx < nq * (k1 - k0); idx += NT) {
    const int kk = idx / nq, q = idx - kk * nq, k = k0 + kk;
    const int s = per_row ? q / R : q;
    if (!live[s] || (per_row && q - s * R >= N[s])) continue;
    const float dx = grad_dot(W + (size_t)k * Op, delta + (size_t)q * ds, O, vec);
    float *o = act + (size_t)q * as + kk;
    *o = RELU ? ebc_cadrl::grad_relu_back(*o, dx) : dx;
  }
}

// a pass's opening: the row counts L.N of its nc states (from c0 on; 0 for the other of the SP places), a barrier, then
// the rows into L.X [slot][Tp], zeros in the slots a state does not have: those are never read from memory.  The caller's
// barrier follows.
template <int NT, class Launch, class Lds>
__device__ __forceinline__ void grad_load_rows(const Launch &a, const Lds &L, long long c0, int nc, int SP, int T) {
  const int tid = threadIdx.x, R = a.R;
  if (tid < SP) L.N[tid] = tid < nc ? ebc_cadrl::clamp_rows(a.n_valid ? a.n_valid[c0 + tid] : (long long)R, R) : 0;
  __syncthreads();
  for (int i = tid; i < nc * R * T; i += NT) {
    const int q = i / T, k = i - q * T, s = q / R, r = q - s * R;
    L.X[q * L.Tp + k] = r < L.N[s] ? a.rows[((size_t)(c0 + s) * R + r) * T + k] : 0.0f;
  }
}

// the values and the seeds from L.OUT, a thread per state (L.LIVE, L.LOSS, L.SEED; a.value when given), a barrier, then
// the chunk's float64 loss and count in state order: thread 0's, going on from the pass before with cont
template <class Launch, class Lds>
__device__ __forceinline__ void grad_seed(const Launch &a, const Lds &L, long long c0, int nc, int SP, bool cont) {
  using namespace ebc_cadrl;
  const int tid = threadIdx.x;
  if (tid < SP) L.LIVE[tid] = 0;
  if (tid < nc) {
    const long long b = c0 + tid;
    const float val = grad_value(L.OUT[tid], L.N[tid]);
    if (a.value) a.value[b] = val;
    const bool live = grad_live(!a.mask || a.mask[b] != 0, L.N[tid]);
    L.LIVE[tid] = live ? 1 : 0;
    if (live) {
      const float d = grad_diff(val, a.target[b]);
      L.LOSS[tid] = grad_loss(d);
      L.SEED[tid] = a.grad_scale * d;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double loss = cont ? a.loss_part[blockIdx.x] : 0.0;
    long long count = cont ? a.count_part[blockIdx.x] : 0;
    for (int s = 0; s < nc; ++s) {
      if (!L.LIVE[s]) continue;
      loss = loss + L.LOSS[s];
      count += 1;
    }
    a.loss_part[blockIdx.x] = loss;
    a.count_part[blockIdx.x] = count;
  }
}

// grad[i] = the float64 sum of the chunks' partials, chunks ascending, rounded once; several launches of the main kernel
// (each with its own run of chunks) continue the float64 sums in acc64.  CANON: a NaN leaves as the rule's one NaN (the
// value networks); without it with the payload it has (SAIL).
template <bool CANON>
__global__ __launch_bounds__(256) void grad_reduce(const float *__restrict__ partial, const double *__restrict__ loss_part,
                                                   const long long *__restrict__ count_part, int chunks, size_t PF, int first, int last,
                                                   double *acc64, float *grad, double *loss_sum, long long *count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < PF) {
    double s = first ? 0.0 : acc64[i];
    for (int c = 0; c < chunks; ++c) s = s + (double)partial[(size_t)c * PF + i];
    if (last) grad[i] = CANON ? ebc_cadrl::canon((float)s) : (float)s;
    else acc64[i] = s;
  }
  if (i == 0) {
    double l = first ? 0.0 : acc64[PF];
    long long n = first ? 0 : reinterpret_cast<long long *>(acc64)[PF + 1];
    for (int c = 0; c < chunks; ++c) {
      l = l + loss_part[c];
      n += count_part[c];
    }
    if (last) {
      *loss_sum = CANON ? ebc_cadrl::canon(l) : l;
      *count = n;
    } else {
      acc64[PF] = l;
      reinterpret_cast<long long *>(acc64)[PF + 1] = n;
    }
  }
}

}  // namespace ebc
