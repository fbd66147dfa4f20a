// ebc_sail_rule.h — the arithmetic of the SAIL policy (rl/policy/sail.py:9-101 ExtendedNetwork, :114-156 predict and
// transform; rl/utils/transform.py:11-20) in float32, ONE definition for the kernel (hipcc, ebc_sail.h) and for the host
// build the tests compare it with (g++, tests/native/sail_host.cc).
//
// Everything here is made of +, -, *, fmaf, comparisons that select, bit operations and one float64 sqrt: no libm / ocml
// exp, no division.  Both builds compile with -ffp-contract=off, so every fusion is the fmaf written below and the two
// builds agree byte for byte.  A NaN that reaches an output is written as the one canonical quiet NaN (canon), so the
// machines' different payloads do not show.  The summation order is fixed here; it is why the network does not go through
// the matrix instruction.
//
// Inputs of one env: robot[9] float64 in FullState order (px, py, vx, vy, radius, gx, gy, v_pref, theta) and ob[N][5]
// float64 (px, py, vx, vy, radius).  Every value is cast to float32 ONCE, as torch.Tensor([...]) does in SAIL.transform
// (sail.py:134-156): robot vector (px, py, vx, vy, gx, gy), frame rows (px, py, vx, vy).
//
//   arrival     reach_destination (simulator/policy/policy.py:44-52) in float64: sqrt(dy*dy + dx*dx) < radius with
//               dy = py - gy, dx = px - gx gives the action (0, 0).  numpy's own norm may fuse that sum, so states ON the
//               boundary may differ from the reference by one rounding: tests keep states away from it.
//   frame       MultiAgentTransform.transform_frame: row i = frame[i] followed by frame[j] - frame[i] for every j != i,
//               j ascending; the subtraction in float32 (4 N values per row).
//   Linear      acc = bias[o]; acc = fmaf(w[o][k], x[k], acc) for k ascending.
//   ReLU        a selection: x < 0 ? 0 : x.  A NaN stays a NaN, as torch's does.
//   softmax     over the N logits of an env (dim = 1): m = the maximum by selection in ascending order (a NaN logit makes
//               every score NaN, as torch's does); e[j] = exp(l[j] - m) by the exp_parts construction of ebc_lstm_cell.h
//               (differences below -87 count as -87); s = e[0] + e[1] + ... ascending; score[j] = e[j] * (1 / s) with the
//               reciprocal built from recip_1_2 on s's mantissa and an exact power of two (1 <= s <= N).
//   crowd       feat_crowd[u] = 0; feat_crowd[u] = fmaf(feat_pairwise[j][u], score[j], feat_crowd[u]) for j ascending.
//   task input  (gx - px, gy - py, vx, vy), subtracted in float32 on the cast values (sail.py:93-95).
//   outputs     action[2] = the planner's two outputs widened to float64 ((0, 0) for an arrived env, NaN for an env whose
//               row count is not N); feat_joint[64] float32 (the network's also for an arrived env; zeros for an env whose
//               row count is not N).
//
// Packed weights: the 14 Linear layers in the order of the Layer enum, each as W[k][64] (unit u of step k at k * 64 + u,
// units past the layer's width zero) followed by its bias[64] (zero past the width): one k step of 64 units is 64 adjacent
// floats.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "ebc_lstm_cell.h"

#if defined(__HIPCC__)
#define EBC_SAIL_HD __host__ __device__ inline
#else
#define EBC_SAIL_HD inline
#endif

#define EBC_SAIL_MIN_ADULTS 2
#define EBC_SAIL_MAX_ADULTS 32
#define EBC_SAIL_LOCAL 32
#define EBC_SAIL_HIDDEN 64
#define EBC_SAIL_LAYERS 14
#ifndef EBC_SAIL_MAX_GROUP
#define EBC_SAIL_MAX_GROUP 8   // envs per workgroup at the most
#endif
#define EBC_SAIL_GROUP_ROWS 48 // adult rows per workgroup at the most (whole envs; one env when N alone exceeds it)

namespace ebc_sail {

// the order of EbcSailWeights.weight / .bias and of the packed image
enum Layer { ROBOT0, ROBOT2, ADULT0, ADULT2, HEAD, EMBED, PAIR0, PAIR2, ATT0, ATT2, TASK0, TASK2, JOINT, PLANNER };

EBC_SAIL_HD int layer_in(int l, int N) {
  return l == ROBOT0 || l == TASK0 ? 4 : l == ROBOT2 ? EBC_SAIL_LOCAL : l == ADULT0 ? 4 * N : l == JOINT ? 2 * EBC_SAIL_HIDDEN : EBC_SAIL_HIDDEN;
}
EBC_SAIL_HD int layer_out(int l) {
  return l == ROBOT0 || l == ROBOT2 || l == HEAD ? EBC_SAIL_LOCAL : l == ATT2 ? 1 : l == PLANNER ? 2 : EBC_SAIL_HIDDEN;
}
// floats before layer l's W in the packed image; its bias follows its W
EBC_SAIL_HD size_t layer_offset(int l, int N) {
  size_t at = 0;
  for (int q = 0; q < l; ++q) at += (size_t)(layer_in(q, N) + 1) * EBC_SAIL_HIDDEN;
  return at;
}
EBC_SAIL_HD size_t packed_floats(int N) { return layer_offset(EBC_SAIL_LAYERS, N); }

// envs a workgroup of the kernel owns (the softmax and the crowd sum stay inside it)
EBC_SAIL_HD int group_envs(int N) {
  const int g = EBC_SAIL_GROUP_ROWS / N;
  return g < 1 ? 1 : (g > EBC_SAIL_MAX_GROUP ? EBC_SAIL_MAX_GROUP : g);
}

// torch layout [out][in] -> the packed image
inline void pack(int N, const float *const *weight, const float *const *bias, float *P) {
  for (int l = 0; l < EBC_SAIL_LAYERS; ++l) {
    const int K = layer_in(l, N), O = layer_out(l);
    float *W = P + layer_offset(l, N), *B = W + (size_t)K * EBC_SAIL_HIDDEN;
    for (int k = 0; k < K; ++k)
      for (int u = 0; u < EBC_SAIL_HIDDEN; ++u) W[(size_t)k * EBC_SAIL_HIDDEN + u] = u < O ? weight[l][(size_t)u * K + k] : 0.0f;
    for (int u = 0; u < EBC_SAIL_HIDDEN; ++u) B[u] = u < O ? bias[l][u] : 0.0f;
  }
}

EBC_SAIL_HD float relu(float x) { return x < 0.0f ? 0.0f : x; }

EBC_SAIL_HD float canon(float x) { return x == x ? x : ebc_lstm::float_of(0x7fc00000u); }
EBC_SAIL_HD double canon(double x) {
  if (x == x) return x;
  const uint64_t u = 0x7ff8000000000000ull;
  double d;
  memcpy(&d, &u, 8);
  return d;
}

// reach_destination in float64 on the uncast state
EBC_SAIL_HD bool arrived(const double *robot) {
  const double dy = robot[1] - robot[6], dx = robot[0] - robot[5];
  return sqrt(dy * dy + dx * dx) < robot[4];
}

// the casts: rv[6] = (px, py, vx, vy, gx, gy), task[4] = (gx - px, gy - py, vx, vy)
EBC_SAIL_HD void robot_vectors(const double *robot, float *rv, float *task) {
  rv[0] = (float)robot[0];
  rv[1] = (float)robot[1];
  rv[2] = (float)robot[2];
  rv[3] = (float)robot[3];
  rv[4] = (float)robot[5];
  rv[5] = (float)robot[6];
  task[0] = rv[4] - rv[0];
  task[1] = rv[5] - rv[1];
  task[2] = rv[2];
  task[3] = rv[3];
}

// element k (0 .. 4 N - 1) of row i of transform_frame(frame [N][4])
EBC_SAIL_HD float frame_input(const float *frame, int i, int k) {
  const int c = k & 3, q = k >> 2;
  if (q == 0) return frame[4 * i + c];
  const int j = q - 1 < i ? q - 1 : q;
  return frame[4 * j + c] - frame[4 * i + c];
}

// one k step of T rows of one unit
template <int T>
EBC_SAIL_HD void unit_step(float (&acc)[T], float w, const float (&x)[T]) {
  for (int t = 0; t < T; ++t) acc[t] = fmaf(w, x[t], acc[t]);
}

// 1 / s for a normal s >= 1; a NaN gives the NaN
EBC_SAIL_HD float recip_sum(float s) {
  const uint32_t b = ebc_lstm::bits_of(s), be = (b >> 23) & 0xffu;
  const float m = ebc_lstm::float_of((b & 0x007fffffu) | 0x3f800000u);  // s's mantissa in [1, 2)
  const float scale = ebc_lstm::float_of(((254u - be) & 0xffu) << 23);    // 2^-(exponent of s), exact
  const float r = ebc_lstm::recip_1_2(m) * scale;
  return s == s ? r : s;
}

// scores of the n logits l[0 .. n) (stride ls) into score[0 .. n)
EBC_SAIL_HD void softmax(const float *l, int ls, int n, float *score) {
  float m = l[0];
  for (int j = 1; j < n; ++j) m = l[(size_t)j * ls] > m ? l[(size_t)j * ls] : m;
  float s = 0.0f;
  for (int j = 0; j < n; ++j) {
    float sc, p;
    ebc_lstm::exp_parts(l[(size_t)j * ls] - m, sc, p);
    const float e = fmaf(sc, p, sc);
    score[j] = e;
    s = j == 0 ? e : s + e;
  }
  const float r = recip_sum(s);
  for (int j = 0; j < n; ++j) score[j] = score[j] * r;
}

// the outputs of an env from the planner's two values: arrived -> (0, 0); rows != N -> NaN
EBC_SAIL_HD double action_of(float planned, bool is_arrived, bool rows_ok) {
  const double nan = canon((double)ebc_lstm::float_of(0x7fc00000u));
  return !rows_ok ? nan : (is_arrived ? 0.0 : canon((double)planned));
}
EBC_SAIL_HD float feature_of(float f, bool rows_ok) { return rows_ok ? canon(f) : 0.0f; }

// y[0 .. O) = (relu of) W x + b of packed layer l, serially; the host build's form of a layer
inline void linear(const float *P, int N, int l, const float *x, float *y, bool with_relu) {
  const int K = layer_in(l, N), O = layer_out(l);
  const float *W = P + layer_offset(l, N), *B = W + (size_t)K * EBC_SAIL_HIDDEN;
  for (int o = 0; o < O; ++o) {
    float acc[1] = {B[o]};
    for (int k = 0; k < K; ++k) {
      const float xk[1] = {x[k]};
      unit_step<1>(acc, W[(size_t)k * EBC_SAIL_HIDDEN + o], xk);
    }
    y[o] = with_relu ? relu(acc[0]) : acc[0];
  }
}

// ONE env, serially (the host build's whole network; the kernel of ebc_sail.h walks the same steps with a unit per lane):
// robot[9], ob [>= N][5] (rows at or past N are not read), n_rows = the env's row count -> action[2], feat_joint[64]
inline void forward_env(const float *P, int N, const double *robot, const double *ob, long long n_rows, double *action, float *feat_joint) {
  constexpr int H = EBC_SAIL_HIDDEN, L = EBC_SAIL_LOCAL, MA = EBC_SAIL_MAX_ADULTS;
  float rv[6], task[4], frame[4 * MA];
  robot_vectors(robot, rv, task);
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < 4; ++c) frame[4 * i + c] = (float)ob[5 * i + c];
  float a[H], b[H], emb_robot[L], joint_in[2 * H];
  linear(P, N, ROBOT0, rv, a, true);
  linear(P, N, ROBOT2, a, emb_robot, true);
  linear(P, N, TASK0, task, a, true);
  linear(P, N, TASK2, a, joint_in, true);
  float feat_pairwise[MA][H], logit[MA], score[MA], x[4 * MA];
  for (int i = 0; i < N; ++i) {
    for (int k = 0; k < 4 * N; ++k) x[k] = frame_input(frame, i, k);
    linear(P, N, ADULT0, x, a, true);
    linear(P, N, ADULT2, a, b, true);
    for (int u = 0; u < L; ++u) a[u] = emb_robot[u];
    linear(P, N, HEAD, b, a + L, true);
    linear(P, N, EMBED, a, b, true);
    linear(P, N, PAIR0, b, a, true);
    linear(P, N, PAIR2, a, feat_pairwise[i], false);
    linear(P, N, ATT0, b, a, true);
    linear(P, N, ATT2, a, logit + i, false);
  }
  softmax(logit, 1, N, score);
  for (int u = 0; u < H; ++u) {
    float acc = 0.0f;
    for (int j = 0; j < N; ++j) acc = fmaf(feat_pairwise[j][u], score[j], acc);
    joint_in[H + u] = acc;
  }
  float fj[H], planned[2];
  linear(P, N, JOINT, joint_in, fj, true);
  linear(P, N, PLANNER, fj, planned, false);
  const bool rows_ok = n_rows == (long long)N, is_arrived = arrived(robot);
  action[0] = action_of(planned[0], is_arrived, rows_ok);
  action[1] = action_of(planned[1], is_arrived, rows_ok);
  if (feat_joint)
    for (int u = 0; u < H; ++u) feat_joint[u] = feature_of(fj[u], rows_ok);
}

}  // namespace ebc_sail
