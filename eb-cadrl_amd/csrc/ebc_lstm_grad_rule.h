// ebc_lstm_grad_rule.h — the gradient of the LSTM-RL value networks' regression loss with respect to their weights, in
// float32: ONE definition for the kernel (hipcc, ebc_lstm_grad.h) and for the host build the tests compare it with (g++,
// tests/native/lstm_grad_host.cc).  The networks are rl/policy/lstm_rl.py:9-69: ValueNetwork1 (rows -> LSTM(T, H) -> mlp on
// cat(rows[0][:S], h_n)) and ValueNetwork2 (rows -> mlp1, four layers, ReLU between, none after the last -> LSTM(mlp1 out,
// H) -> mlp); mlp has four layers and one output.  It builds on the scalar steps of ebc_cadrl_grad_rule.h (chain, grad_relu,
// grad_relu_back, grad_live, grad_diff, grad_loss, grad_value, canon, clamp_rows, pad4) and on the cell of ebc_lstm_cell.h
// (lstm_sigmoid, lstm_tanh) and changes nothing there.
//
// Made of + - *, fmaf, comparisons, selections and bit operations; both builds compile with -ffp-contract=off and agree
// byte for byte.  Every NaN that leaves (value, joint, loss_sum, grad) is the one quiet NaN of ebc_cadrl_rule.h.
//
//   unit        acc = 0, then acc = fmaf(x[k], W[k][u], acc) for k ascending, then acc + bias[u]; ReLU is x < 0 ? 0 : x.
//   rows        n = clamp_rows(n_valid, R): above R counts as R, below 0 as 0; steps at or past n are never read.
//   mlp1        (ValueNetwork2) per row t < n: a1 = relu(L0 x), a2 = relu(L1 a1), a3 = relu(L2 a2), xi = L3 a3;
//               ValueNetwork1: xi = the row itself.  I is xi's width.
//   gates       per step t < n and gate row q (torch's order: i rows 0 .. H, f, g, o): pre = b_ih[q] + b_hh[q] (one float32
//               addition), then pre = fmaf(w_ih[q][k], xi[t][k], pre) for k ascending over I, then
//               pre = fmaf(w_hh[q][k], h[t-1][k], pre) for k ascending over H on top of it; h[-1] = c[-1] = 0 (the terms are
//               taken, as ebc_lstm_cell.h takes them).
//   cell        i, f, o = lstm_sigmoid(pre), g = lstm_tanh(pre); c[t] = fmaf(f, c[t-1], i * g); tc = lstm_tanh(c[t]);
//               h[t] = o * tc: ebc_lstm_cell.h's cell_update, with what the backward needs kept (i, f, g, o, c, tc, h).
//   mlp         j = cat(x[0][0 .. S), h[n-1]); m1 = relu(L4 j), m2 = relu(L5 m1), m3 = relu(L6 m2), out = L7 m3.
//   value       n >= 1 ? canon(out) : NaN; joint[k] = canon(j[k]) for n >= 1 and 0 without rows.
//   live, loss, seed   as ebc_cadrl_grad_rule.h: live = mask != 0 (or no mask) and n >= 1, by selection; d = value - target;
//               the loss is (double)d * (double)d; delta_out = grad_scale * d.
//   Linear      dW[k][u] = fmaf(delta[u], x[k], dW[k][u]); db[u] = db[u] + delta[u];
//               dx[k] = 0, then dx[k] = fmaf(W[k][u], delta[u], dx[k]) for u ascending; ReLU: out > 0 ? d : 0.
//   time        dh = L4's dx at the inputs S .., dc = 0; then for t = n-1 down to 0, per unit (cell_back):
//                 dcs = fmaf(dh * o, 1 - tc * tc, dc)            1 - y * y is fmaf(-y, y, 1)
//                 d_o = (dh * tc) * (o * (1 - o))                d_i = (dcs * g) * (i * (1 - i))
//                 d_f = (dcs * c[t-1]) * (f * (1 - f))           d_g = (dcs * i) * (1 - g * g)
//                 dc  = dcs * f                                  the step's delta[q] = (d_i | d_f | d_g | d_o), kept
//               and, for t >= 1, dh[k] = 0, then dh[k] = fmaf(w_hh[q][k], delta[q], dh[k]) for q ascending over all 4 H rows.
//   cell'       AFTER the walk, from the kept deltas: dw_ih[q][k] = fmaf(delta[t][q], xi[t][k], .), dw_hh[q][k] =
//               fmaf(delta[t][q], h[t-1][k], .), db_ih[q] = db_hh[q] = . + delta[t][q], for t ASCENDING 0 .. n-1: the one order
//               of time steps inside a state, for mlp1's layers too.  b_ih and b_hh are two tensors with the same gradient
//               bytes, not one fused bias: an optimizer with per-entry state (Adam) moves them as it moves torch's.
//   mlp1'       dxi[t][k] = 0, then fmaf(w_ih[q][k], delta[t][q], .) for q ascending; L3 .. L0 backward per row, ReLU masks
//               a3, a2, a1.
//
// Summation over samples.  The batch is cut into chunks of EBC_LSTM_GRAD_CHUNK consecutive states.  Inside a chunk every
// weight's chain starts at 0 and runs over the live states ascending and, for the layers that see rows (mlp1 and the cell),
// over a state's steps ascending.  The chunks' float32 partials are added in ascending chunk order in float64 and rounded to
// float32 once; the chunks' losses likewise, kept in float64.  Nothing else enters.  A chain is at most CHUNK * R terms
// long.
//
// What is shared and what is written twice: as in ebc_cadrl_grad_rule.h.  The scalar steps are shared; the LOOPS exist
// serially here (the host build) and in parallel in ebc_lstm_grad.h, held together by the byte comparison of
// tests/test_lstm_train_gpu.py.
//
// Packed image (weights and gradient alike): mlp1's four layers (ValueNetwork1: none), then the cell as w_ih[k][4 H] (gate
// row q of input k at k * 4 H + q), w_hh[k][4 H], b_ih[4 H], b_hh[4 H], then mlp's four layers; a Linear layer as W[k][Op] —
// unit u of input k at k * Op + u, Op = the layer's units padded to a multiple of 4 — followed by bias[Op]; pad entries
// exactly 0.  At the reference widths (T 13, S 6, mlp1 150, 100, 100, 50, H 50, mlp 150, 100, 100, 1) 87 248 floats with
// mlp1 and 47 268 without.
#pragma once

#include <stddef.h>

#include <vector>

#include "ebc_cadrl_grad_rule.h"
#include "ebc_lstm_cell.h"

#define EBC_LSTM_GRAD_CHUNK 4        // states per chunk: a float32 chain is at most 4 R terms long before float64 takes over
#define EBC_LSTM_GRAD_LAYERS 8       // Linear layers: mlp1 (4, or absent) + mlp (4)
#define EBC_LSTM_GRAD_MAX_IN 64      // widest row
#define EBC_LSTM_GRAD_MAX_WIDTH 256  // widest Linear layer
#define EBC_LSTM_GRAD_MAX_CHUNKS 256 // chunks one launch of the kernel takes (89 MB of partials at the reference widths)

namespace ebc_lstmg {

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

enum { L_M1A = 0, L_M1B, L_M1C, L_M1D, L_MA, L_MB, L_MC, L_MD };

struct GradDims {
  int T, S, I, H, two;  // row width, self state entries, the cell's input width, its units, with mlp1 (ValueNetwork2)
  int K[EBC_LSTM_GRAD_LAYERS], O[EBC_LSTM_GRAD_LAYERS], Op[EBC_LSTM_GRAD_LAYERS];  // mlp1's are 0 without mlp1
  unsigned at[EBC_LSTM_GRAD_LAYERS];  // where layer l's W starts in the packed image, in floats
  unsigned at_cell;                   // where w_ih starts: w_ih [I][4H] | w_hh [H][4H] | b_ih [4H] | b_hh [4H]
  unsigned floats;
};

// widths[10]: the row width, mlp1's four units (ignored without mlp1), H, mlp's four units
EBC_CADRL_HD GradDims grad_dims(const int *widths, int self_dim, int two) {
  GradDims D;
  D.T = widths[0], D.S = self_dim, D.two = two ? 1 : 0, D.H = widths[5];
  D.I = D.two ? widths[4] : widths[0];
  unsigned at = 0;
  for (int l = 0; l < EBC_LSTM_GRAD_LAYERS; ++l) {
    int K = 0, O = 0;
    if (l < 4 && D.two) K = widths[l], O = widths[l + 1];
    if (l == 4) K = self_dim + D.H, O = widths[6];
    if (l > 4) K = widths[l + 1], O = widths[l + 2];
    if (l == 4) {
      D.at_cell = at;
      at += (unsigned)(D.I + D.H + 2) * 4u * (unsigned)D.H;
    }
    D.K[l] = K, D.O[l] = O, D.Op[l] = pad4(O);
    D.at[l] = at;
    at += O ? (unsigned)(K + 1) * (unsigned)D.Op[l] : 0u;
  }
  D.floats = at;
  return D;
}

// 0 = fine; 1: the row width; 2 .. 5: a layer of mlp1 outside 1 .. 256; 6: the cell's input wider than EBC_LSTM_MAX_DIM;
// 7: H outside 1 .. EBC_LSTM_MAX_DIM; 8 .. 11: a layer of mlp outside 1 .. 256, or a last layer that is not one unit wide;
// 12: the self state does not fit the row
EBC_CADRL_HD int grad_dims_refused(const int *widths, int self_dim, int two) {
  if (widths[0] < 1 || widths[0] > EBC_LSTM_GRAD_MAX_IN) return 1;
  if (two) {
    for (int l = 1; l <= 4; ++l)
      if (widths[l] < 1 || widths[l] > EBC_LSTM_GRAD_MAX_WIDTH) return l + 1;
    if (widths[4] > EBC_LSTM_MAX_DIM) return 6;
  } else if (widths[0] > EBC_LSTM_MAX_DIM) {
    return 6;
  }
  if (widths[5] < 1 || widths[5] > EBC_LSTM_MAX_DIM) return 7;
  for (int l = 6; l <= 9; ++l)
    if (widths[l] < 1 || widths[l] > EBC_LSTM_GRAD_MAX_WIDTH || (l == 9 && widths[l] != 1)) return l + 2;
  return self_dim < 0 || self_dim > widths[0] ? 12 : 0;
}

// ---- the cell's scalar steps
EBC_CADRL_HD float gate_bias(float b_ih, float b_hh) { return b_ih + b_hh; }
EBC_CADRL_HD float gate_chain(float w, float v, float acc) { return __builtin_fmaf(w, v, acc); }
// what a unit's step keeps: i, f, g, o, c, tanh(c), h — ebc_lstm::cell_update's operations
EBC_CADRL_HD void cell_forward(float pi, float pf, float pg, float po, float c_prev, float &gi, float &gf, float &gg, float &go, float &c,
                               float &tc, float &h) {
  gi = ebc_lstm::lstm_sigmoid(pi), gf = ebc_lstm::lstm_sigmoid(pf), gg = ebc_lstm::lstm_tanh(pg), go = ebc_lstm::lstm_sigmoid(po);
  c = __builtin_fmaf(gf, c_prev, gi * gg);
  tc = ebc_lstm::lstm_tanh(c);
  h = go * tc;
}
EBC_CADRL_HD float d_sigmoid(float y) { return y * (1.0f - y); }
EBC_CADRL_HD float d_tanh(float y) { return __builtin_fmaf(-y, y, 1.0f); }
// a unit's step backward: dh, dc (of this step's h and c) and what the step kept -> the four gate deltas and dc of c[t-1]
EBC_CADRL_HD void cell_back(float dh, float dc, float gi, float gf, float gg, float go, float tc, float c_prev, float &di, float &df, float &dg,
                            float &dout, float &dc_prev) {
  const float dcs = __builtin_fmaf(dh * go, d_tanh(tc), dc);
  dout = (dh * tc) * d_sigmoid(go);
  di = (dcs * gg) * d_sigmoid(gi);
  df = (dcs * c_prev) * d_sigmoid(gf);
  dg = (dcs * gi) * d_tanh(gg);
  dc_prev = dcs * gf;
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

// what the forward of one state keeps for its backward; steps side by side, MAX_WIDTH apart (the cell's: MAX_DIM)
struct StateActs {
  int n;
  std::vector<float> a1, a2, a3, xi, gate, c, tc, h, j, m1, m2, m3;
  explicit StateActs(int R)
      : n(0), a1((size_t)R * 256), a2((size_t)R * 256), a3((size_t)R * 256), xi((size_t)R * 256), gate((size_t)R * 4 * EBC_LSTM_MAX_DIM),
        c((size_t)R * EBC_LSTM_MAX_DIM), tc((size_t)R * EBC_LSTM_MAX_DIM), h((size_t)R * EBC_LSTM_MAX_DIM), j(EBC_LSTM_GRAD_MAX_IN + EBC_LSTM_MAX_DIM),
        m1(256), m2(256), m3(256) {}
};

// the forward of ONE state with n >= 1 rows x[t][0 .. T) -> L7's output
inline float grad_forward_state(const float *P, const GradDims &D, const float *x, int n, StateActs &A) {
  const int I = D.I, H = D.H, H4 = 4 * D.H, MD = EBC_LSTM_MAX_DIM;
  const float *w_ih = P + D.at_cell, *w_hh = w_ih + (size_t)I * H4, *b_ih = w_hh + (size_t)H * H4, *b_hh = b_ih + H4;
  const float zero[EBC_LSTM_MAX_DIM] = {0.0f};
  A.n = n;
  for (int t = 0; t < n; ++t) {
    float *xi = &A.xi[(size_t)t * 256];
    if (D.two) {
      grad_layer(P, D, L_M1A, x + (size_t)t * D.T, &A.a1[(size_t)t * 256], true);
      grad_layer(P, D, L_M1B, &A.a1[(size_t)t * 256], &A.a2[(size_t)t * 256], true);
      grad_layer(P, D, L_M1C, &A.a2[(size_t)t * 256], &A.a3[(size_t)t * 256], true);
      grad_layer(P, D, L_M1D, &A.a3[(size_t)t * 256], xi, false);
    } else {
      for (int k = 0; k < I; ++k) xi[k] = x[(size_t)t * D.T + k];
    }
    const float *hp = t ? &A.h[(size_t)(t - 1) * MD] : zero, *cp = t ? &A.c[(size_t)(t - 1) * MD] : zero;
    float *g = &A.gate[(size_t)t * 4 * MD];
    for (int q = 0; q < H4; ++q) {
      float pre = gate_bias(b_ih[q], b_hh[q]);
      for (int k = 0; k < I; ++k) pre = gate_chain(w_ih[(size_t)k * H4 + q], xi[k], pre);
      for (int k = 0; k < H; ++k) pre = gate_chain(w_hh[(size_t)k * H4 + q], hp[k], pre);
      g[q] = pre;
    }
    for (int u = 0; u < H; ++u)
      cell_forward(g[u], g[H + u], g[2 * H + u], g[3 * H + u], cp[u], g[u], g[H + u], g[2 * H + u], g[3 * H + u], A.c[(size_t)t * MD + u],
                   A.tc[(size_t)t * MD + u], A.h[(size_t)t * MD + u]);
  }
  for (int k = 0; k < D.S; ++k) A.j[k] = x[k];
  for (int k = 0; k < H; ++k) A.j[D.S + k] = A.h[(size_t)(n - 1) * MD + k];
  grad_layer(P, D, L_MA, A.j.data(), A.m1.data(), true);
  grad_layer(P, D, L_MB, A.m1.data(), A.m2.data(), true);
  grad_layer(P, D, L_MC, A.m2.data(), A.m3.data(), true);
  return grad_unit(P, D, L_MD, 0, A.m3.data());
}

// the backward of ONE live state from its seed into the chunk's partial G; the gates of A are overwritten by their
// deltas and mlp1's activations by theirs, as the kernel overwrites them
inline void grad_backward_state(const float *P, float *G, const GradDims &D, const float *x, StateActs &A, float seed) {
  const int I = D.I, H = D.H, H4 = 4 * D.H, MD = EBC_LSTM_MAX_DIM, n = A.n;
  const float *w_ih = P + D.at_cell, *w_hh = w_ih + (size_t)I * H4;
  float *g_ih = G + D.at_cell, *g_hh = g_ih + (size_t)I * H4, *gb_ih = g_hh + (size_t)H * H4, *gb_hh = gb_ih + H4;
  const float zero[EBC_LSTM_MAX_DIM] = {0.0f};
  float d[256], dj[EBC_LSTM_GRAD_MAX_IN + EBC_LSTM_MAX_DIM], dh[EBC_LSTM_MAX_DIM], dc[EBC_LSTM_MAX_DIM];
  grad_linear(P, G, D, L_MD, A.m3.data(), &seed, d);
  for (int k = 0; k < D.K[L_MD]; ++k) A.m3[k] = grad_relu_back(A.m3[k], d[k]);
  grad_linear(P, G, D, L_MC, A.m2.data(), A.m3.data(), d);
  for (int k = 0; k < D.K[L_MC]; ++k) A.m2[k] = grad_relu_back(A.m2[k], d[k]);
  grad_linear(P, G, D, L_MB, A.m1.data(), A.m2.data(), d);
  for (int k = 0; k < D.K[L_MB]; ++k) A.m1[k] = grad_relu_back(A.m1[k], d[k]);
  grad_linear(P, G, D, L_MA, A.j.data(), A.m1.data(), dj);
  for (int k = 0; k < H; ++k) dh[k] = dj[D.S + k], dc[k] = 0.0f;
  // the walk back through time: the gates become their deltas
  for (int t = n - 1; t >= 0; --t) {
    float *g = &A.gate[(size_t)t * 4 * MD];
    const float *cp = t ? &A.c[(size_t)(t - 1) * MD] : zero;
    for (int u = 0; u < H; ++u)
      cell_back(dh[u], dc[u], g[u], g[H + u], g[2 * H + u], g[3 * H + u], A.tc[(size_t)t * MD + u], cp[u], g[u], g[H + u], g[2 * H + u],
                g[3 * H + u], dc[u]);
    if (t == 0) break;
    for (int k = 0; k < H; ++k) {
      float acc = 0.0f;
      for (int q = 0; q < H4; ++q) acc = chain(w_hh[(size_t)k * H4 + q], g[q], acc);
      dh[k] = acc;
    }
  }
  // the cell's weights, steps ascending
  for (int t = 0; t < n; ++t) {
    const float *g = &A.gate[(size_t)t * 4 * MD], *xi = &A.xi[(size_t)t * 256], *hp = t ? &A.h[(size_t)(t - 1) * MD] : zero;
    for (int k = 0; k < I; ++k)
      for (int q = 0; q < H4; ++q) g_ih[(size_t)k * H4 + q] = chain(g[q], xi[k], g_ih[(size_t)k * H4 + q]);
    for (int k = 0; k < H; ++k)
      for (int q = 0; q < H4; ++q) g_hh[(size_t)k * H4 + q] = chain(g[q], hp[k], g_hh[(size_t)k * H4 + q]);
    for (int q = 0; q < H4; ++q) gb_ih[q] = gb_ih[q] + g[q], gb_hh[q] = gb_hh[q] + g[q];
  }
  if (!D.two) return;
  // mlp1, steps ascending
  for (int t = 0; t < n; ++t) {
    const float *g = &A.gate[(size_t)t * 4 * MD];
    float *xi = &A.xi[(size_t)t * 256], *a3 = &A.a3[(size_t)t * 256], *a2 = &A.a2[(size_t)t * 256], *a1 = &A.a1[(size_t)t * 256];
    for (int k = 0; k < I; ++k) {
      float acc = 0.0f;
      for (int q = 0; q < H4; ++q) acc = chain(w_ih[(size_t)k * H4 + q], g[q], acc);
      xi[k] = acc;
    }
    grad_linear(P, G, D, L_M1D, a3, xi, d);
    for (int k = 0; k < D.K[L_M1D]; ++k) a3[k] = grad_relu_back(a3[k], d[k]);
    grad_linear(P, G, D, L_M1C, a2, a3, d);
    for (int k = 0; k < D.K[L_M1C]; ++k) a2[k] = grad_relu_back(a2[k], d[k]);
    grad_linear(P, G, D, L_M1B, a1, a2, d);
    for (int k = 0; k < D.K[L_M1B]; ++k) a1[k] = grad_relu_back(a1[k], d[k]);
    grad_linear(P, G, D, L_M1A, x + (size_t)t * D.T, a1, nullptr);
  }
}

// The whole batch, serially: rows [B][R][T], n_valid [B] or null = R, target [B], sample_mask [B] or null -> grad
// [D.floats], loss_sum, count, and when wanted value [B] and joint [B][S + H]
inline void grad_batch(const float *P, const GradDims &D, int B, int R, const float *rows, const long long *n_valid, const float *target,
                       const unsigned char *sample_mask, float grad_scale, float *grad, double *loss_sum, long long *count, float *value,
                       float *joint) {
  const size_t PF = D.floats;
  const int T = D.T, J = D.S + D.H;
  std::vector<double> total(PF, 0.0);
  std::vector<float> G(PF);
  StateActs A(R > 0 ? R : 1);
  double loss = 0.0;
  long long live_states = 0;
  for (int c0 = 0; c0 < B; c0 += EBC_LSTM_GRAD_CHUNK) {
    const int c1 = c0 + EBC_LSTM_GRAD_CHUNK < B ? c0 + EBC_LSTM_GRAD_CHUNK : B;
    for (size_t i = 0; i < PF; ++i) G[i] = 0.0f;
    double chunk_loss = 0.0;
    for (int b = c0; b < c1; ++b) {
      const float *rb = rows + (size_t)b * R * T;
      const int n = clamp_rows(n_valid ? n_valid[b] : (long long)R, R);
      const float val = grad_value(n >= 1 ? grad_forward_state(P, D, rb, n, A) : 0.0f, n);
      if (value) value[b] = val;
      if (joint)
        for (int k = 0; k < J; ++k) joint[(size_t)b * J + k] = n >= 1 ? canon(A.j[k]) : 0.0f;
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

// torch's layout -> the packed image P[D.floats], pad entries 0: weight / bias [8] of the Linear layers in the packed order
// (mlp1's four are not read without mlp1), [out][in] / [out]; the cell's w_ih [4H][I], w_hh [4H][H], b_ih [4H], b_hh [4H]
inline void grad_pack(const GradDims &D, const float *const *weight, const float *const *bias, const float *w_ih, const float *w_hh,
                      const float *b_ih, const float *b_hh, float *P) {
  for (unsigned i = 0; i < D.floats; ++i) P[i] = 0.0f;
  for (int l = 0; l < EBC_LSTM_GRAD_LAYERS; ++l) {
    float *W = P + D.at[l];
    for (int k = 0; k < D.K[l]; ++k)
      for (int u = 0; u < D.O[l]; ++u) W[(size_t)k * D.Op[l] + u] = weight[l][(size_t)u * D.K[l] + k];
    for (int u = 0; u < D.O[l]; ++u) W[(size_t)D.K[l] * D.Op[l] + u] = bias[l][u];
  }
  const int I = D.I, H = D.H, H4 = 4 * D.H;
  float *c = P + D.at_cell;
  for (int k = 0; k < I; ++k)
    for (int q = 0; q < H4; ++q) c[(size_t)k * H4 + q] = w_ih[(size_t)q * I + k];
  c += (size_t)I * H4;
  for (int k = 0; k < H; ++k)
    for (int q = 0; q < H4; ++q) c[(size_t)k * H4 + q] = w_hh[(size_t)q * H + k];
  c += (size_t)H * H4;
  for (int q = 0; q < H4; ++q) c[q] = b_ih[q], c[H4 + q] = b_hh[q];
}

}  // namespace ebc_lstmg
