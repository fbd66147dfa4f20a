// ebc_sarl_grad_rule.h — the gradient of the SARL value network's regression loss with respect to its weights, in float32:
// ONE definition for the kernel (hipcc, ebc_sarl_grad.h) and for the host build the tests compare it with (g++,
// tests/native/sarl_grad_host.cc).  The network is rl/policy/sarl.py:38-82: mlp1 (2 layers, ReLU after both), mlp2 (2 layers,
// no last ReLU), the mean of mlp1's output over a state's rows (with_global_state), attention (3 layers, one score per
// row), the reference's masked softmax, the weighted sum of mlp2's features, mlp3 (4 layers, one output) on
// cat(self state, weighted feature).  It builds on the scalar steps of ebc_cadrl_grad_rule.h (chain, grad_relu,
// grad_relu_back, grad_live, grad_diff, grad_loss, grad_value, canon, clamp_rows, pad4) and changes nothing there.
//
// Made of + - *, fmaf, float64 division, comparisons, selections and bit operations; both builds compile with
// -ffp-contract=off and agree byte for byte.  Every NaN that leaves (value, attention, loss_sum, grad) is the one quiet NaN
// of ebc_cadrl_rule.h.
//
//   unit        acc = 0, then acc = fmaf(x[k], W[k][u], acc) for k ascending, then acc + bias[u]; ReLU is x < 0 ? 0 : x.
//   rows        n = clamp_rows(n_valid, R): above R counts as R, below 0 as 0; rows at or past n are never read.
//   mlp1, mlp2  per row r < n: a1 = relu(L0 x), h1 = relu(L1 a1), b1 = relu(L2 h1), ft = L3 b1.
//   mean        g[k] = (float)((double)(0 + h1[0][k] + h1[1][k] + ... in float32, r ascending) / (double)n).
//   attention   per row: c1 = relu(L4 [h1 | g]) as ONE chain (k over h1 first, then over g; without global state over h1
//               alone), c2 = relu(L5 c1), s = L6 c2 (one unit).
//   softmax     e[r] = s[r] != 0 ? exp(s[r]) : 0 (no maximum subtracted, as the reference; a NaN score gives NaN);
//               exp(s) = sc * (1 + p) = fmaf(sc, p, sc) from ebc_lstm::exp_parts on s clamped to [-87, 88];
//               sum = 0 + e[0] + e[1] + ... in float32; w[r] = (float)((double)e[r] / (double)sum): float64 division is
//               the correctly rounded one in both builds.  A sum of 0 gives NaN weights, as the reference's 0 / 0.
//   weighted    wf[f] = 0, then wf[f] = fmaf(w[r], ft[r][f], wf[f]) for r ascending.
//   mlp3        j = cat(x[0][0 .. S), wf); m1 = relu(L7 j), m2 = relu(L8 m1), m3 = relu(L9 m2), out = L10 m3.
//   value       n >= 1 ? canon(out) : NaN; attention[r] = canon(w[r]) for r < n and 0 for r >= n.
//   live, loss, seed   as ebc_cadrl_grad_rule.h: live = mask != 0 (or no mask) and n >= 1, by selection; d = value - target;
//               the loss is (double)d * (double)d; delta_out = grad_scale * d.
//   Linear      dW[k][u] = fmaf(delta[u], x[k], dW[k][u]); db[u] = db[u] + delta[u];
//               dx[k] = 0, then dx[k] = fmaf(W[k][u], delta[u], dx[k]) for u ascending; ReLU: out > 0 ? d : 0.
//   weighted'   dwf = dx of L7 at the inputs S ..; dft[r][f] = w[r] * dwf[f].
//   softmax'    c[r] = chain over f ascending of dwf[f] * (ft[r][f] - wf[f]) from 0; m = chain over r ascending of
//               w[r] * c[r] from 0; ds[r] = w[r] * (c[r] - m).  That is w[r] * (q[r] - sum_j w[j] q[j]), q[r] = dwf . ft[r],
//               with the difference taken per feature BEFORE the product: rows with similar features (the usual case) would
//               cancel most digits of q[r] - the sum.  m is 0 but for rounding (that of wf above all); taking it off
//               keeps sum_r ds[r] at 0, which the last attention layer's gradient, a sum of cancelling terms, depends on.
//               The (s != 0) factor is a constant inside w, so a score of exactly 0 passes nothing on.
//   mean'       dg[k] = 0 + t[0][k] + t[1][k] + ..., r ascending, t[r][k] = L4's dx at input H + k of row r;
//               dm[k] = (float)((double)dg[k] / (double)n) goes to every row < n.
//   h1'         dh1[r][k] = relu_back(h1[r][k], (L2's dx + L4's dx at input k) + dm[k]); without global state the sum of the two.
//
// A wide row (OM-SARL: the occupancy map behind the rotated columns, up to 224 floats) is a longer ascending chain in layer
// 0 and a longer dW there, and nothing else: no other step sees the row's width.
//
// Summation over samples.  The batch is cut into chunks of EBC_SARL_GRAD_CHUNK consecutive states.  Inside a chunk every
// weight's chain starts at 0 and runs over the live states ascending and, for the layers that see rows (0 .. 6), over a
// state's rows ascending.  The chunks' float32 partials are added in ascending chunk order in float64 and rounded to float32
// once; the chunks' losses likewise, kept in float64.  Nothing else enters.  A chain is at most CHUNK * R terms long: 40
// at R = 10.
//
// What is shared and what is written twice: as in ebc_cadrl_grad_rule.h.  The scalar steps are shared; the LOOPS exist
// serially here (the host build) and in parallel in ebc_sarl_grad.h, held together by the byte comparison of
// tests/test_sarl_train_gpu.py.
//
// Packed image (weights and gradient alike): the eleven layers in the order mlp1.0, mlp1.2, mlp2.0, mlp2.2, attention.0,
// attention.2, attention.4, mlp3.0, mlp3.2, mlp3.4, mlp3.6; layer l as W[k][Op] — unit u of input k at k * Op + u, Op = the
// layer's units padded to a multiple of 4 — followed by bias[Op]; pad entries exactly 0.  97 452 floats at the reference
// widths (T 13; 150, 100; 100, 50; 100, 100, 1; 150, 100, 100, 1; global state; self state 6).
#pragma once

#include <stddef.h>

#include <vector>

#include "ebc_cadrl_grad_rule.h"
#include "ebc_lstm_cell.h"

#define EBC_SARL_GRAD_CHUNK 4        // states per chunk: a float32 chain is at most 4 R terms long before float64 takes over
#define EBC_SARL_GRAD_LAYERS 11      // 2 + 2 + 3 + 4
#define EBC_SARL_GRAD_MAX_IN 64      // widest rotated row
#define EBC_SARL_GRAD_MAX_OM 192     // widest occupancy map appended to a row (EBC_OM_MAX_WIDTH)
#define EBC_SARL_GRAD_MAX_WIDE 224   // widest row with its map (EBC_OM_MAX_ROW_WIDTH: what the deciding blocks take)
#define EBC_SARL_GRAD_MAX_ROW 256    // what the host build's buffers hold of a row, wide or not
#define EBC_SARL_GRAD_MAX_WIDTH 256  // widest hidden layer
#define EBC_SARL_GRAD_MAX_CHUNKS 256 // chunks one launch of the kernel takes (100 MB of partials at the reference widths)
// The layer form (ebc_sarl_grad_layers.h): the same rule layer by layer over the whole batch, activations in device memory
#define EBC_SARL_GRAD_LAYERS_MAX_WIDTH 640    // widest hidden layer of the layer form (the reference's policy_x4: 600)
#define EBC_SARL_GRAD_LAYERS_MAX_ROWS 128     // most row slots per state of the layer form (the product's row limit)
#define EBC_SARL_GRAD_LAYERS_RUN_SLOTS 65536  // row slots (states * R, whole chunks) of one run of the layer form
// What the serial loops below hold of a hidden layer, per row: the stride of their buffers.  It moves no byte of any
// result; a host build with -DEBC_SARL_GRAD_HOST_WIDTH=640 runs the networks of the layer form.
#ifndef EBC_SARL_GRAD_HOST_WIDTH
#define EBC_SARL_GRAD_HOST_WIDTH 256
#endif

namespace ebc_sarl {

using ebc_cadrl::canon;
using ebc_cadrl::chain;
using ebc_cadrl::clamp_rows;
using ebc_cadrl::grad_diff;
using ebc_cadrl::grad_live;
using ebc_cadrl::grad_loss;
using ebc_cadrl::grad_relu;
using ebc_cadrl::grad_relu_back;
using ebc_cadrl::grad_value;
using ebc_cadrl::pad4;

enum { L_M1A = 0, L_M1B, L_M2A, L_M2B, L_ATA, L_ATB, L_ATC, L_M3A, L_M3B, L_M3C, L_M3D };

struct GradDims {
  int T, S, global;  // row width, self state entries, with_global_state
  int K[EBC_SARL_GRAD_LAYERS], O[EBC_SARL_GRAD_LAYERS], Op[EBC_SARL_GRAD_LAYERS];
  unsigned at[EBC_SARL_GRAD_LAYERS];  // where layer l's W starts in the packed image, in floats
  unsigned floats;
};

// widths[12]: the row width, then the units of mlp1 (2), mlp2 (2), attention (3), mlp3 (4)
EBC_CADRL_HD GradDims grad_dims(const int *widths, int self_dim, int global) {
  GradDims D;
  D.T = widths[0], D.S = self_dim, D.global = global ? 1 : 0;
  unsigned at = 0;
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l) {
    int K = widths[l];
    if (l == L_ATA) K = widths[2] * (D.global ? 2 : 1);
    if (l == L_M3A) K = self_dim + widths[4];
    D.K[l] = K;
    D.O[l] = widths[l + 1];
    D.Op[l] = pad4(widths[l + 1]);
    D.at[l] = at;
    at += (unsigned)(K + 1) * (unsigned)D.Op[l];
  }
  D.floats = at;
  return D;
}

// 0 = fine; 1: the row width; 2 .. 12: the units of layer (code - 2) outside 1 .. 256, or a last layer that is not one
// unit wide; 13: the self state does not fit the row
EBC_CADRL_HD int grad_dims_refused(const int *widths, int self_dim) {
  if (widths[0] < 1 || widths[0] > EBC_SARL_GRAD_MAX_IN) return 1;
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l) {
    const int o = widths[l + 1];
    if (o < 1 || o > EBC_SARL_GRAD_MAX_WIDTH) return l + 2;
    if ((l == L_ATC || l == L_M3D) && o != 1) return l + 2;
  }
  return self_dim < 0 || self_dim > widths[0] ? 13 : 0;
}

// The network of OM-SARL: widths[0] = the rotated width T, and the rows the gradient reads are T + om_width wide (the maps
// follow the rotated columns; the self state stays inside the first T).  grad_dims_refused's codes on the rotated widths,
// and 14: om_width outside 0 .. 192; 15: T + om_width above 224.  Its dims are grad_dims on widths with [0] = T + om_width.
EBC_CADRL_HD int grad_dims_refused_wide(const int *widths, int self_dim, int om_width) {
  const int bad = grad_dims_refused(widths, self_dim);
  if (bad) return bad;
  if (om_width < 0 || om_width > EBC_SARL_GRAD_MAX_OM) return 14;
  return widths[0] + om_width > EBC_SARL_GRAD_MAX_WIDE ? 15 : 0;
}

// The layer form's limits: grad_dims_refused_wide's codes with 640 as the widest hidden layer; the rows' limits are the same.
EBC_CADRL_HD int grad_dims_refused_layers(const int *widths, int self_dim, int om_width) {
  if (widths[0] < 1 || widths[0] > EBC_SARL_GRAD_MAX_IN) return 1;
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l) {
    const int o = widths[l + 1];
    if (o < 1 || o > EBC_SARL_GRAD_LAYERS_MAX_WIDTH) return l + 2;
    if ((l == L_ATC || l == L_M3D) && o != 1) return l + 2;
  }
  if (self_dim < 0 || self_dim > widths[0]) return 13;
  if (om_width < 0 || om_width > EBC_SARL_GRAD_MAX_OM) return 14;
  return widths[0] + om_width > EBC_SARL_GRAD_MAX_WIDE ? 15 : 0;
}

// exp(s) of a score
EBC_CADRL_HD float score_exp(float s) {
  float sc, p;
  ebc_lstm::exp_parts(s > 88.0f ? 88.0f : s, sc, p);
  return s != 0.0f ? __builtin_fmaf(sc, p, sc) : 0.0f;
}
EBC_CADRL_HD float quotient(float a, float b) { return (float)((double)a / (double)b); }
EBC_CADRL_HD float over_rows(float a, int n) { return (float)((double)a / (double)n); }
EBC_CADRL_HD float centred(float ft, float wf) { return ft - wf; }
EBC_CADRL_HD float score_back(float w, float c, float m) { return w * (c - m); }
EBC_CADRL_HD float h1_back(float h1, float d2, float d4, float dm, int global) {
  const float s = d2 + d4;
  return grad_relu_back(h1, global ? s + dm : s);
}

// unit u of layer l on the inputs x[0 .. K)
EBC_CADRL_HD float grad_unit(const float *P, const GradDims &D, int l, int u, const float *x) {
  const float *W = P + D.at[l];
  const int K = D.K[l], Op = D.Op[l];
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) acc = chain(x[k], W[(size_t)k * Op + u], acc);
  return acc + W[(size_t)K * Op + u];
}

inline void grad_layer(const float *P, const GradDims &D, int l, const float *x, float *y, bool relu) {
  for (int u = 0; u < D.O[l]; ++u) {
    const float v = grad_unit(P, D, l, u, x);
    y[u] = relu ? grad_relu(v) : v;
  }
}

// one sample of layer l: the chains of G continue with delta[0 .. O) and x[0 .. K); dx[0 .. K) when wanted
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

enum { HW = EBC_SARL_GRAD_HOST_WIDTH };

// what the forward of one state keeps for its backward; rows side by side, HW apart ([h1 | g]: 2 HW)
struct StateActs {
  int n;
  std::vector<float> a1, h1, b1, ft, c1, c2, xa, s, w, g, j, m1, m2, m3;
  explicit StateActs(int R)
      : n(0), a1((size_t)R * HW), h1((size_t)R * HW), b1((size_t)R * HW), ft((size_t)R * HW), c1((size_t)R * HW), c2((size_t)R * HW),
        xa((size_t)R * 2 * HW), s(R), w(R), g(HW), j(EBC_SARL_GRAD_MAX_ROW + HW), m1(HW), m2(HW), m3(HW) {}
};

// the forward of ONE state with n >= 1 rows x[r][0 .. T) -> L10's output
inline float grad_forward_state(const float *P, const GradDims &D, const float *x, int n, StateActs &A) {
  const int H = D.O[L_M1B], F = D.O[L_M2B];
  A.n = n;
  for (int r = 0; r < n; ++r) {
    grad_layer(P, D, L_M1A, x + (size_t)r * D.T, &A.a1[(size_t)r * HW], true);
    grad_layer(P, D, L_M1B, &A.a1[(size_t)r * HW], &A.h1[(size_t)r * HW], true);
    grad_layer(P, D, L_M2A, &A.h1[(size_t)r * HW], &A.b1[(size_t)r * HW], true);
    grad_layer(P, D, L_M2B, &A.b1[(size_t)r * HW], &A.ft[(size_t)r * HW], false);
  }
  if (D.global)
    for (int k = 0; k < H; ++k) {
      float acc = 0.0f;
      for (int r = 0; r < n; ++r) acc = acc + A.h1[(size_t)r * HW + k];
      A.g[k] = over_rows(acc, n);
    }
  float sum = 0.0f;
  for (int r = 0; r < n; ++r) {
    float *xa = &A.xa[(size_t)r * 2 * HW];
    for (int k = 0; k < H; ++k) xa[k] = A.h1[(size_t)r * HW + k];
    if (D.global)
      for (int k = 0; k < H; ++k) xa[H + k] = A.g[k];
    grad_layer(P, D, L_ATA, xa, &A.c1[(size_t)r * HW], true);
    grad_layer(P, D, L_ATB, &A.c1[(size_t)r * HW], &A.c2[(size_t)r * HW], true);
    A.s[r] = grad_unit(P, D, L_ATC, 0, &A.c2[(size_t)r * HW]);
    A.w[r] = score_exp(A.s[r]);
    sum = sum + A.w[r];
  }
  for (int r = 0; r < n; ++r) A.w[r] = quotient(A.w[r], sum);
  for (int k = 0; k < D.S; ++k) A.j[k] = x[k];
  for (int f = 0; f < F; ++f) {
    float acc = 0.0f;
    for (int r = 0; r < n; ++r) acc = chain(A.w[r], A.ft[(size_t)r * HW + f], acc);
    A.j[D.S + f] = acc;
  }
  grad_layer(P, D, L_M3A, A.j.data(), A.m1.data(), true);
  grad_layer(P, D, L_M3B, A.m1.data(), A.m2.data(), true);
  grad_layer(P, D, L_M3C, A.m2.data(), A.m3.data(), true);
  return grad_unit(P, D, L_M3D, 0, A.m3.data());
}

// the backward of ONE live state from its seed into the chunk's partial G; the activations of A are overwritten by
// their deltas, as the kernel overwrites them
inline void grad_backward_state(const float *P, float *G, const GradDims &D, const float *x, StateActs &A, float seed) {
  const int H = D.O[L_M1B], F = D.O[L_M2B], n = A.n;
  float d[2 * HW], dj[EBC_SARL_GRAD_MAX_ROW + HW];
  grad_linear(P, G, D, L_M3D, A.m3.data(), &seed, d);
  for (int k = 0; k < D.K[L_M3D]; ++k) A.m3[k] = grad_relu_back(A.m3[k], d[k]);
  grad_linear(P, G, D, L_M3C, A.m2.data(), A.m3.data(), d);
  for (int k = 0; k < D.K[L_M3C]; ++k) A.m2[k] = grad_relu_back(A.m2[k], d[k]);
  grad_linear(P, G, D, L_M3B, A.m1.data(), A.m2.data(), d);
  for (int k = 0; k < D.K[L_M3B]; ++k) A.m1[k] = grad_relu_back(A.m1[k], d[k]);
  grad_linear(P, G, D, L_M3A, A.j.data(), A.m1.data(), dj);
  const float *dwf = dj + D.S;
  // the weighted sum and the softmax
  for (int r = 0; r < n; ++r) {
    float acc = 0.0f;
    for (int f = 0; f < F; ++f) acc = chain(dwf[f], centred(A.ft[(size_t)r * HW + f], A.j[D.S + f]), acc);
    A.s[r] = acc;
  }
  float m = 0.0f;
  for (int r = 0; r < n; ++r) m = chain(A.w[r], A.s[r], m);
  for (int r = 0; r < n; ++r) {
    A.s[r] = score_back(A.w[r], A.s[r], m);
    for (int f = 0; f < F; ++f) A.ft[(size_t)r * HW + f] = A.w[r] * dwf[f];
  }
  // mlp2
  for (int r = 0; r < n; ++r) {
    float *b1 = &A.b1[(size_t)r * HW];
    grad_linear(P, G, D, L_M2B, b1, &A.ft[(size_t)r * HW], d);
    for (int k = 0; k < D.K[L_M2B]; ++k) b1[k] = grad_relu_back(b1[k], d[k]);
  }
  for (int r = 0; r < n; ++r) grad_linear(P, G, D, L_M2A, &A.h1[(size_t)r * HW], &A.b1[(size_t)r * HW], nullptr);
  // attention
  for (int r = 0; r < n; ++r) {
    float *c2 = &A.c2[(size_t)r * HW];
    grad_linear(P, G, D, L_ATC, c2, &A.s[r], d);
    for (int k = 0; k < D.K[L_ATC]; ++k) c2[k] = grad_relu_back(c2[k], d[k]);
  }
  for (int r = 0; r < n; ++r) {
    float *c1 = &A.c1[(size_t)r * HW];
    grad_linear(P, G, D, L_ATB, c1, &A.c2[(size_t)r * HW], d);
    for (int k = 0; k < D.K[L_ATB]; ++k) c1[k] = grad_relu_back(c1[k], d[k]);
  }
  for (int r = 0; r < n; ++r) grad_linear(P, G, D, L_ATA, &A.xa[(size_t)r * 2 * HW], &A.c1[(size_t)r * HW], nullptr);
  // h1: mlp2's layer 0, attention's layer 0 and the mean
  const float *W2 = P + D.at[L_M2A], *W4 = P + D.at[L_ATA];
  const int O2 = D.O[L_M2A], Op2 = D.Op[L_M2A], O4 = D.O[L_ATA], Op4 = D.Op[L_ATA];
  std::vector<float> dm(H, 0.0f);
  if (D.global)
    for (int k = 0; k < H; ++k) {
      float dg = 0.0f;
      for (int r = 0; r < n; ++r) {
        float acc = 0.0f;
        for (int u = 0; u < O4; ++u) acc = chain(W4[(size_t)(H + k) * Op4 + u], A.c1[(size_t)r * HW + u], acc);
        dg = dg + acc;
      }
      dm[k] = over_rows(dg, n);
    }
  for (int r = 0; r < n; ++r) {  // L_M2A and L_ATA have read h1 (xa holds its copy): its delta takes its place
    float *h1 = &A.h1[(size_t)r * HW];
    for (int k = 0; k < H; ++k) {
      float d2 = 0.0f, d4 = 0.0f;
      for (int u = 0; u < O2; ++u) d2 = chain(W2[(size_t)k * Op2 + u], A.b1[(size_t)r * HW + u], d2);
      for (int u = 0; u < O4; ++u) d4 = chain(W4[(size_t)k * Op4 + u], A.c1[(size_t)r * HW + u], d4);
      h1[k] = h1_back(h1[k], d2, d4, dm[k], D.global);
    }
  }
  for (int r = 0; r < n; ++r) {
    float *a1 = &A.a1[(size_t)r * HW];
    grad_linear(P, G, D, L_M1B, a1, &A.h1[(size_t)r * HW], d);
    for (int k = 0; k < D.K[L_M1B]; ++k) a1[k] = grad_relu_back(a1[k], d[k]);
  }
  for (int r = 0; r < n; ++r) grad_linear(P, G, D, L_M1A, x + (size_t)r * D.T, &A.a1[(size_t)r * HW], nullptr);
}

// The whole batch, serially: rows [B][R][T], n_valid [B] or null = R, target [B], sample_mask [B] or null -> grad
// [D.floats], loss_sum, count, and when wanted value [B] and attention [B][R]
inline void grad_batch(const float *P, const GradDims &D, int B, int R, const float *rows, const long long *n_valid, const float *target,
                       const unsigned char *sample_mask, float grad_scale, float *grad, double *loss_sum, long long *count, float *value,
                       float *attention) {
  const size_t PF = D.floats;
  const int T = D.T;
  std::vector<double> total(PF, 0.0);
  std::vector<float> G(PF);
  StateActs A(R > 0 ? R : 1);
  double loss = 0.0;
  long long live_states = 0;
  for (int c0 = 0; c0 < B; c0 += EBC_SARL_GRAD_CHUNK) {
    const int c1 = c0 + EBC_SARL_GRAD_CHUNK < B ? c0 + EBC_SARL_GRAD_CHUNK : B;
    for (size_t i = 0; i < PF; ++i) G[i] = 0.0f;
    double chunk_loss = 0.0;
    for (int b = c0; b < c1; ++b) {
      const float *rb = rows + (size_t)b * R * T;
      const int n = clamp_rows(n_valid ? n_valid[b] : (long long)R, R);
      const float val = grad_value(n >= 1 ? grad_forward_state(P, D, rb, n, A) : 0.0f, n);
      if (value) value[b] = val;
      if (attention)
        for (int r = 0; r < R; ++r) attention[(size_t)b * R + r] = r < n ? canon(A.w[r]) : 0.0f;
      if (!grad_live(!sample_mask || sample_mask[b] != 0, n)) continue;
      const float d = grad_diff(val, target[b]);
      chunk_loss = chunk_loss + grad_loss(d);
      live_states += 1;
      grad_backward_state(P, G.data(), D, rb, A, grad_scale * d);
    }
    for (size_t i = 0; i < PF; ++i) total[i] = total[i] + (double)G[i];
    loss = loss + chunk_loss;
  }
  for (size_t i = 0; i < PF; ++i) grad[i] = canon((float)total[i]);
  *loss_sum = canon(loss);
  *count = live_states;
}

// torch's layout (weight [out][in], bias [out], per layer in the packed order) -> the packed image P[D.floats], pad entries 0
inline void grad_pack(const GradDims &D, const float *const *weight, const float *const *bias, float *P) {
  for (unsigned i = 0; i < D.floats; ++i) P[i] = 0.0f;
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l) {
    float *W = P + D.at[l];
    for (int k = 0; k < D.K[l]; ++k)
      for (int u = 0; u < D.O[l]; ++u) W[(size_t)k * D.Op[l] + u] = weight[l][(size_t)u * D.K[l] + k];
    for (int u = 0; u < D.O[l]; ++u) W[(size_t)D.K[l] * D.Op[l] + u] = bias[l][u];
  }
}

}  // namespace ebc_sarl
