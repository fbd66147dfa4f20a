// ebc_cadrl_grad_rule.h — the gradient of the CADRL value network's regression loss with respect to its weights, in
// float32: ONE definition for the kernel (hipcc, ebc_cadrl_grad.h) and for the host build the tests compare it with
// (g++, tests/native/cadrl_grad_host.cc).  It adds to ebc_cadrl_rule.h (the minimum over a state's rows) and changes
// nothing there.  The network is four Linear layers ending in one output (rl/policy/cadrl.py:13-31), ReLU after the
// first three.
//
// Made of + - *, fmaf, comparisons, selections and bit operations; both builds compile with -ffp-contract=off and agree
// byte for byte.  Every NaN that leaves (value, loss_sum, grad) is the one quiet NaN of ebc_cadrl_rule.h: an x86 host
// and the GPU give an invalid operation's NaN different signs.
//
//   forward     of ONE row: a unit's pre-activation is acc = 0, then acc = fmaf(x[k], W[k][u], acc) for k ascending, then
//               acc + bias[u]; ReLU (x < 0 ? 0 : x: a NaN stays, as in torch) after layers 1-3; layer 4 is one such chain.
//               This fixes the forward's bytes FOR THIS HEADER.  They are not promised to be the bytes of
//               ebc_mlp2_forward_f32, whose one-output tail adds its partial sums in an order that depends on the launch
//               form: the trainer's `value` and the deciding blocks' values agree to float32 rounding, not bit for bit.
//   value       of a state: min_rows of ebc_cadrl_rule.h over its rows [0, n), n = clamp_rows(n_valid, R): NaN
//               propagating, n_valid above R counts as R and below 0 as 0, rows at or past n are never read; no row gives
//               NaN.  min_row is the FIRST row that holds the minimum (of a NaN minimum: the first NaN row), -1 without
//               rows.  The gradient goes through that row alone: its activations are the ones kept.
//   live        sample_mask != 0 (or no mask) and n >= 1.  Masking is by SELECTION: a state that is not live enters no
//               sum, so a NaN anywhere in it reaches nothing but its own `value`.  A NaN inside a live state reaches
//               loss_sum and grad.
//   loss        d = value - target in float32; a state's loss is (double)d * (double)d (exact); a chunk's loss is the
//               float64 sum of its live states' losses, state ascending.
//   seed        delta_out = grad_scale * d: grad is d/dweights of grad_scale / 2 * loss_sum, the convention of
//               ebc_sail_grad_rule.h; grad_scale = 2 / count is torch's MSELoss over count values.
//   Linear      dW[k][u] = fmaf(delta[u], x[k], dW[k][u]);  db[u] = db[u] + delta[u];
//               dx[k] = 0, then dx[k] = fmaf(W[k][u], delta[u], dx[k]) for u ascending.
//   ReLU        delta_pre = out > 0 ? delta_out : 0 (torch's subgradient at 0 is 0).
//
// Summation over samples.  The batch is cut into chunks of EBC_CADRL_GRAD_CHUNK consecutive states.  Inside a chunk every
// weight's chain above starts at 0 and runs over the live states ascending.  The chunks' float32 partials are added in
// ascending chunk order in float64 and rounded to float32 once; the chunks' losses likewise, kept in float64.  Nothing
// else enters: not the number of workgroups, the rows a workgroup takes at once, or a chunk's place in the grid.
//
// What is shared and what is written twice.  The kernel compiles the scalar steps of this header (chain, grad_relu,
// grad_relu_back, grad_diff, grad_loss, grad_value, grad_live, canon, min_rows, first_min_row, grad_dims, pad4).  The LOOPS
// around them exist twice: serially here (grad_unit, grad_forward_row, grad_linear, grad_backward_state, grad_batch: the
// host build) and in parallel in ebc_cadrl_grad.h (cadrl_layer, cadrl_dw, cadrl_dx, the chunk's loss) and ebc_grad_common.h
// (grad_reduce).
// Editing a loop here does not change the kernel: the two are held together by the byte comparison of
// tests/test_cadrl_train_gpu.py alone, and a change of order must be made in both.
//
// Packed image (weights and gradient alike): the four layers in order, layer l as W[k][Op] — unit u of input k at
// k * Op + u, Op = the layer's units padded to a multiple of 4 — followed by bias[Op]; pad entries exactly 0.
#pragma once

#include <stddef.h>

#include <vector>

#include "ebc_cadrl_rule.h"

#define EBC_CADRL_GRAD_CHUNK 16      // a float32 chain is at most 16 terms long before float64 takes over
#define EBC_CADRL_GRAD_LAYERS 4
#define EBC_CADRL_GRAD_MAX_IN 64     // widest row the gradient takes
#define EBC_CADRL_GRAD_MAX_WIDTH 256 // widest hidden layer (the reference's are 150, 100, 100)

namespace ebc_cadrl {

struct GradDims {
  int K[EBC_CADRL_GRAD_LAYERS], O[EBC_CADRL_GRAD_LAYERS], Op[EBC_CADRL_GRAD_LAYERS];  // inputs, units, units padded
  unsigned at[EBC_CADRL_GRAD_LAYERS];  // where layer l's W starts in the packed image, in floats
  unsigned floats;                     // of the packed image
};

EBC_CADRL_HD int pad4(int n) { return (n + 3) & ~3; }

// widths[5]: the row width, then the four layers' units
EBC_CADRL_HD GradDims grad_dims(const int *widths) {
  GradDims D;
  unsigned at = 0;
  for (int l = 0; l < EBC_CADRL_GRAD_LAYERS; ++l) {
    D.K[l] = widths[l];
    D.O[l] = widths[l + 1];
    D.Op[l] = pad4(widths[l + 1]);
    D.at[l] = at;
    at += (unsigned)(D.K[l] + 1) * (unsigned)D.Op[l];
  }
  D.floats = at;
  return D;
}

// what the gradient takes: 0 = fine, else the index of the first width outside its limit plus 1
EBC_CADRL_HD int grad_dims_refused(const int *widths) {
  if (widths[0] < 1 || widths[0] > EBC_CADRL_GRAD_MAX_IN) return 1;
  for (int l = 1; l < EBC_CADRL_GRAD_LAYERS; ++l)
    if (widths[l] < 1 || widths[l] > EBC_CADRL_GRAD_MAX_WIDTH) return l + 1;
  return widths[EBC_CADRL_GRAD_LAYERS] == 1 ? 0 : EBC_CADRL_GRAD_LAYERS + 1;
}

EBC_CADRL_HD float canon(float x) { return x != x ? nan_f32() : x; }
EBC_CADRL_HD double canon(double x) { return x != x ? nan_f64() : x; }
EBC_CADRL_HD float grad_relu(float x) { return x < 0.0f ? 0.0f : x; }
EBC_CADRL_HD float grad_relu_back(float out, float d) { return out > 0.0f ? d : 0.0f; }
EBC_CADRL_HD bool grad_live(bool sample, int n) { return sample && n >= 1; }
EBC_CADRL_HD float grad_diff(float value, float target) { return value - target; }
EBC_CADRL_HD double grad_loss(float d) { return (double)d * (double)d; }
EBC_CADRL_HD float grad_value(float out, int n) { return n >= 1 ? canon(out) : nan_f32(); }

// the first row of v[0 .. n) that holds m = min_rows(v, n, 1): of a NaN minimum the first NaN row; -1 without rows
EBC_CADRL_HD int first_min_row(const float *v, int n, float m) {
  for (int r = 0; r < n; ++r) {
    const float x = v[r];
    if (x == m || (m != m && x != x)) return r;
  }
  return -1;
}

// one step of a unit's chain, of a dW chain and of a dx chain: the same fused operation
EBC_CADRL_HD float chain(float a, float b, float acc) { return __builtin_fmaf(a, b, acc); }

// unit u of a layer W[k][Op] | bias[Op] on the inputs x[0 .. K)
EBC_CADRL_HD float grad_unit(const float *W, int K, int Op, int u, const float *x) {
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) acc = chain(x[k], W[(size_t)k * Op + u], acc);
  return acc + W[(size_t)K * Op + u];
}

// the forward of one row x[0 .. K[0]); a1, a2, a3: the three ReLU outputs (what the backward keeps) -> layer 4's output
inline float grad_forward_row(const float *P, const GradDims &D, const float *x, float *a1, float *a2, float *a3) {
  float *out[3] = {a1, a2, a3};
  const float *in = x;
  for (int l = 0; l < 3; ++l) {
    for (int u = 0; u < D.O[l]; ++u) out[l][u] = grad_relu(grad_unit(P + D.at[l], D.K[l], D.Op[l], u, in));
    in = out[l];
  }
  return grad_unit(P + D.at[3], D.K[3], D.Op[3], 0, in);
}

// one sample of layer l: delta[0 .. O) and the layer's input x[0 .. K) continue the chains of G (a chunk's partial,
// packed layout); dx[0 .. K), when wanted, is the gradient with respect to x
inline void grad_linear(const float *P, float *G, const GradDims &D, int l, const float *x, const float *delta, float *dx) {
  const int K = D.K[l], O = D.O[l], Op = D.Op[l];
  const float *W = P + D.at[l];
  float *GW = G + D.at[l], *GB = GW + (size_t)K * Op;
  for (int k = 0; k < K; ++k)
    for (int u = 0; u < O; ++u) GW[(size_t)k * Op + u] = chain(delta[u], x[k], GW[(size_t)k * Op + u]);
  for (int u = 0; u < O; ++u) GB[u] = GB[u] + delta[u];
  if (!dx) return;
  for (int k = 0; k < K; ++k) {
    float acc = 0.0f;
    for (int u = 0; u < O; ++u) acc = chain(W[(size_t)k * Op + u], delta[u], acc);
    dx[k] = acc;
  }
}

// the backward of ONE live state from its seed, through the kept row's activations, into the chunk's partial G
inline void grad_backward_state(const float *P, float *G, const GradDims &D, const float *x, const float *a1, const float *a2,
                                const float *a3, float seed) {
  float d3[EBC_CADRL_GRAD_MAX_WIDTH], d2[EBC_CADRL_GRAD_MAX_WIDTH], d1[EBC_CADRL_GRAD_MAX_WIDTH];
  grad_linear(P, G, D, 3, a3, &seed, d3);
  for (int k = 0; k < D.K[3]; ++k) d3[k] = grad_relu_back(a3[k], d3[k]);
  grad_linear(P, G, D, 2, a2, d3, d2);
  for (int k = 0; k < D.K[2]; ++k) d2[k] = grad_relu_back(a2[k], d2[k]);
  grad_linear(P, G, D, 1, a1, d2, d1);
  for (int k = 0; k < D.K[1]; ++k) d1[k] = grad_relu_back(a1[k], d1[k]);
  grad_linear(P, G, D, 0, x, d1, nullptr);
}

// The whole batch, serially (the host build; the kernel of ebc_cadrl_grad.h walks the same chains): rows [B][R][T] with
// T = K[0], n_valid [B] or null = R, target [B], sample_mask [B] or null -> grad [D.floats], loss_sum, count, and when
// wanted value [B] and min_row [B]
inline void grad_batch(const float *P, const GradDims &D, int B, int R, const float *rows, const long long *n_valid, const float *target,
                       const unsigned char *sample_mask, float grad_scale, float *grad, double *loss_sum, long long *count, float *value,
                       int *min_row) {
  const size_t PF = D.floats;
  const int T = D.K[0];
  std::vector<double> total(PF, 0.0);
  std::vector<float> G(PF), v(R > 0 ? R : 1);
  float a1[EBC_CADRL_GRAD_MAX_WIDTH], a2[EBC_CADRL_GRAD_MAX_WIDTH], a3[EBC_CADRL_GRAD_MAX_WIDTH];
  double loss = 0.0;
  long long live_states = 0;
  for (int c0 = 0; c0 < B; c0 += EBC_CADRL_GRAD_CHUNK) {
    const int c1 = c0 + EBC_CADRL_GRAD_CHUNK < B ? c0 + EBC_CADRL_GRAD_CHUNK : B;
    for (size_t i = 0; i < PF; ++i) G[i] = 0.0f;
    double chunk_loss = 0.0;
    for (int b = c0; b < c1; ++b) {
      const float *rb = rows + (size_t)b * R * T;
      const int n = clamp_rows(n_valid ? n_valid[b] : (long long)R, R);
      for (int r = 0; r < n; ++r) v[r] = grad_forward_row(P, D, rb + (size_t)r * T, a1, a2, a3);
      const int pick = first_min_row(v.data(), n, min_rows(v.data(), n, 1));
      // the kept row again: the same chains, the same bytes
      const float val = grad_value(pick >= 0 ? grad_forward_row(P, D, rb + (size_t)pick * T, a1, a2, a3) : 0.0f, n);
      if (value) value[b] = val;
      if (min_row) min_row[b] = pick;
      if (!grad_live(!sample_mask || sample_mask[b] != 0, n)) continue;
      const float d = grad_diff(val, target[b]);
      chunk_loss = chunk_loss + grad_loss(d);
      live_states += 1;
      grad_backward_state(P, G.data(), D, rb + (size_t)pick * T, a1, a2, a3, grad_scale * d);
    }
    for (size_t i = 0; i < PF; ++i) total[i] = total[i] + (double)G[i];
    loss = loss + chunk_loss;
  }
  for (size_t i = 0; i < PF; ++i) grad[i] = canon((float)total[i]);
  *loss_sum = canon(loss);
  *count = live_states;
}

// torch's layout (weight [out][in], bias [out], per layer) -> the packed image P[D.floats], pad entries 0
inline void grad_pack(const GradDims &D, const float *const *weight, const float *const *bias, float *P) {
  for (unsigned i = 0; i < D.floats; ++i) P[i] = 0.0f;
  for (int l = 0; l < EBC_CADRL_GRAD_LAYERS; ++l) {
    float *W = P + D.at[l];
    for (int k = 0; k < D.K[l]; ++k)
      for (int u = 0; u < D.O[l]; ++u) W[(size_t)k * D.Op[l] + u] = weight[l][(size_t)u * D.K[l] + k];
    for (int u = 0; u < D.O[l]; ++u) W[(size_t)D.K[l] * D.Op[l] + u] = bias[l][u];
  }
}

}  // namespace ebc_cadrl
