// ebc_sail_grad_rule.h — the gradient of the SAIL network's imitation loss with respect to its weights, in float32: ONE
// definition for the kernel (hipcc, ebc_sail_grad.h) and for the host build the tests compare it with (g++,
// tests/native/sail_grad_host.cc).  It adds to ebc_sail_rule.h and changes nothing there: the forward half is that
// header's, chain for chain, so `planned` has the bytes of ebc_sail_forward.
//
// Made of + - *, fmaf, selections and bit operations; both builds compile with -ffp-contract=off and agree byte for byte.
//
//   w_e         1 unless the env has arrived (ebc_sail::arrived: the forward's action is the constant (0, 0) there), its
//               row count is not N, or sample_mask[e] == 0.  Masking is by SELECTION: an env with w_e = 0 enters no sum,
//               so a NaN or an infinity anywhere in it reaches nothing but its own `action`.
//   loss        l_e = d0 * d0 + d1 * d1 in float64 with d_c = planned[c] - (float)target[c] in float32 (the two products
//               are exact); a chunk's loss is the float64 sum of its live envs' l_e, env ascending.
//   seed        delta_action[c] = grad_scale * d_c.
//   Linear      dW[o][k] = fmaf(delta[o], x[k], dW[o][k]);  db[o] = db[o] + delta[o];
//               dx[k] = 0, then dx[k] = fmaf(W[o][k], delta[o], dx[k]) for o ascending.
//   ReLU        delta_pre = out > 0 ? delta_out : 0 (torch's subgradient at 0 is 0).
//   crowd       dFP[j][u] = dC[u] * score[j];  dscore[j] = 0, then fmaf(dC[u], feat_pairwise[j][u], dscore[j]), u ascending.
//   softmax     exact, scores from the forward: dot = 0, then fmaf(score[j], dscore[j], dot), j ascending;
//               dlogit[j] = score[j] * (dscore[j] - dot).
//   embedding   dEmb = (pairwise path) + (attention path), then joint_embedding's ReLU.
//   emb_robot   the first 32 inputs of joint_embedding: s = 0, then s = s + d[row], the env's rows ascending.
//
// Summation over samples.  The batch is cut into chunks of EBC_SAIL_GRAD_CHUNK consecutive envs.  Inside a chunk every
// weight's chain above starts at 0 and runs over the live envs ascending (for the row layers over (env, row) ascending).
// The chunks' float32 partials are added in ascending chunk order in float64 and rounded to float32 once; the chunks'
// loss sums likewise, kept in float64.  Nothing else enters: not the number of workgroups, the envs a workgroup takes at
// once, or a chunk's place in the grid.  The gradient has the layout of ebc_sail::pack, pad entries exactly 0.
#pragma once

#include <vector>

#include "ebc_sail_rule.h"

// 16 envs: at 4096 envs the grid has 256 workgroups (one per compute unit of an MI355X), and a float32 chain is at most
// 16 * 32 = 512 terms long before float64 takes over
#define EBC_SAIL_GRAD_CHUNK 16
#define EBC_SAIL_GRAD_ROWS 32  // adult rows a workgroup of the kernel keeps on chip at once (whole envs)

namespace ebc_sail {

// envs a workgroup of the gradient kernel takes at once (a chunk is walked in such groups; the sums do not depend on it)
EBC_SAIL_HD int grad_group_envs(int N) {
  const int g = EBC_SAIL_GRAD_ROWS / N;
  return g < 1 ? 1 : (g > EBC_SAIL_MAX_GROUP ? EBC_SAIL_MAX_GROUP : g);
}

EBC_SAIL_HD bool grad_live(const double *robot, long long n_rows, int N, bool sample) {
  return sample && n_rows == (long long)N && !arrived(robot);
}
EBC_SAIL_HD float grad_diff(float planned, double target) { return planned - (float)target; }
EBC_SAIL_HD double grad_loss(float d0, float d1) { return (double)d0 * (double)d0 + (double)d1 * (double)d1; }
EBC_SAIL_HD float relu_back(float out, float d) { return out > 0.0f ? d : 0.0f; }
EBC_SAIL_HD float softmax_back(float score, float dscore, float dot) { return score * (dscore - dot); }

// every activation of one env the backward needs
struct GradActs {
  float rv[6], task[4], r1[EBC_SAIL_LOCAL], r2[EBC_SAIL_LOCAL], t1[EBC_SAIL_HIDDEN], jin[2 * EBC_SAIL_HIDDEN], fj[EBC_SAIL_HIDDEN], planned[2];
  float x[EBC_SAIL_MAX_ADULTS][4 * EBC_SAIL_MAX_ADULTS], a1[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN], a2[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN],
      cat[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN], emb[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN], p1[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN],
      fp[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN], q1[EBC_SAIL_MAX_ADULTS][EBC_SAIL_HIDDEN], logit[EBC_SAIL_MAX_ADULTS], score[EBC_SAIL_MAX_ADULTS];
};

// forward_env of ebc_sail_rule.h, chain for chain, keeping every layer's output
inline void grad_forward_env(const float *P, int N, const double *robot, const double *ob, GradActs &a) {
  constexpr int H = EBC_SAIL_HIDDEN, L = EBC_SAIL_LOCAL, MA = EBC_SAIL_MAX_ADULTS;
  float frame[4 * MA];
  robot_vectors(robot, a.rv, a.task);
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < 4; ++c) frame[4 * i + c] = (float)ob[5 * i + c];
  linear(P, N, ROBOT0, a.rv, a.r1, true);
  linear(P, N, ROBOT2, a.r1, a.r2, true);
  linear(P, N, TASK0, a.task, a.t1, true);
  linear(P, N, TASK2, a.t1, a.jin, true);
  for (int i = 0; i < N; ++i) {
    for (int k = 0; k < 4 * N; ++k) a.x[i][k] = frame_input(frame, i, k);
    linear(P, N, ADULT0, a.x[i], a.a1[i], true);
    linear(P, N, ADULT2, a.a1[i], a.a2[i], true);
    for (int u = 0; u < L; ++u) a.cat[i][u] = a.r2[u];
    linear(P, N, HEAD, a.a2[i], a.cat[i] + L, true);
    linear(P, N, EMBED, a.cat[i], a.emb[i], true);
    linear(P, N, PAIR0, a.emb[i], a.p1[i], true);
    linear(P, N, PAIR2, a.p1[i], a.fp[i], false);
    linear(P, N, ATT0, a.emb[i], a.q1[i], true);
    linear(P, N, ATT2, a.q1[i], a.logit + i, false);
  }
  softmax(a.logit, 1, N, a.score);
  for (int u = 0; u < H; ++u) {
    float acc = 0.0f;
    for (int j = 0; j < N; ++j) acc = fmaf(a.fp[j][u], a.score[j], acc);
    a.jin[H + u] = acc;
  }
  linear(P, N, JOINT, a.jin, a.fj, true);
  linear(P, N, PLANNER, a.fj, a.planned, false);
}

// one sample of packed layer l: delta[0 .. O) and the layer's input x[0 .. K) continue the chains of G (a chunk's
// partial, packed layout); dx[0 .. K), when wanted, is the gradient with respect to x
inline void grad_linear(const float *P, float *G, int N, int l, const float *x, const float *delta, float *dx) {
  const int K = layer_in(l, N), O = layer_out(l);
  const size_t at = layer_offset(l, N);
  const float *W = P + at;
  float *GW = G + at, *GB = GW + (size_t)K * EBC_SAIL_HIDDEN;
  for (int k = 0; k < K; ++k)
    for (int o = 0; o < O; ++o) GW[(size_t)k * EBC_SAIL_HIDDEN + o] = fmaf(delta[o], x[k], GW[(size_t)k * EBC_SAIL_HIDDEN + o]);
  for (int o = 0; o < O; ++o) GB[o] = GB[o] + delta[o];
  if (!dx) return;
  for (int k = 0; k < K; ++k) {
    float acc = 0.0f;
    for (int o = 0; o < O; ++o) acc = fmaf(W[(size_t)k * EBC_SAIL_HIDDEN + o], delta[o], acc);
    dx[k] = acc;
  }
}

// the backward of ONE live env from its seed into the chunk's partial G
inline void grad_backward_env(const float *P, float *G, int N, const GradActs &a, const float *seed) {
  constexpr int H = EBC_SAIL_HIDDEN, L = EBC_SAIL_LOCAL, MA = EBC_SAIL_MAX_ADULTS;
  float dfj[H], djin[2 * H], dt1[H], d[H], e[H];
  grad_linear(P, G, N, PLANNER, a.fj, seed, dfj);
  for (int u = 0; u < H; ++u) dfj[u] = relu_back(a.fj[u], dfj[u]);
  grad_linear(P, G, N, JOINT, a.jin, dfj, djin);
  for (int u = 0; u < H; ++u) djin[u] = relu_back(a.jin[u], djin[u]);
  grad_linear(P, G, N, TASK2, a.t1, djin, dt1);
  for (int u = 0; u < H; ++u) dt1[u] = relu_back(a.t1[u], dt1[u]);
  grad_linear(P, G, N, TASK0, a.task, dt1, nullptr);
  const float *dC = djin + H;
  float dscore[MA], dlogit[MA], dot = 0.0f;
  for (int j = 0; j < N; ++j) {
    float s = 0.0f;
    for (int u = 0; u < H; ++u) s = fmaf(dC[u], a.fp[j][u], s);
    dscore[j] = s;
  }
  for (int j = 0; j < N; ++j) dot = fmaf(a.score[j], dscore[j], dot);
  for (int j = 0; j < N; ++j) dlogit[j] = softmax_back(a.score[j], dscore[j], dot);
  // the layers of the rows: every layer walks the env's rows ascending, so each weight's chain is in (env, row) order
  float dcat[MA][H], da[MA][H];
  for (int j = 0; j < N; ++j) {
    float demb[H];
    for (int u = 0; u < H; ++u) d[u] = dC[u] * a.score[j];
    grad_linear(P, G, N, PAIR2, a.p1[j], d, e);
    for (int u = 0; u < H; ++u) e[u] = relu_back(a.p1[j][u], e[u]);
    grad_linear(P, G, N, PAIR0, a.emb[j], e, demb);
    grad_linear(P, G, N, ATT2, a.q1[j], dlogit + j, e);
    for (int u = 0; u < H; ++u) e[u] = relu_back(a.q1[j][u], e[u]);
    grad_linear(P, G, N, ATT0, a.emb[j], e, d);
    for (int u = 0; u < H; ++u) demb[u] = relu_back(a.emb[j][u], demb[u] + d[u]);
    grad_linear(P, G, N, EMBED, a.cat[j], demb, dcat[j]);
    for (int u = 0; u < H; ++u) dcat[j][u] = relu_back(a.cat[j][u], dcat[j][u]);
    grad_linear(P, G, N, HEAD, a.a2[j], dcat[j] + L, da[j]);
    for (int u = 0; u < H; ++u) da[j][u] = relu_back(a.a2[j][u], da[j][u]);
    grad_linear(P, G, N, ADULT2, a.a1[j], da[j], e);
    for (int u = 0; u < H; ++u) e[u] = relu_back(a.a1[j][u], e[u]);
    grad_linear(P, G, N, ADULT0, a.x[j], e, nullptr);
  }
  float dr2[L], dr1[L];
  for (int u = 0; u < L; ++u) {
    float s = 0.0f;
    for (int j = 0; j < N; ++j) s = s + dcat[j][u];
    dr2[u] = s;
  }
  grad_linear(P, G, N, ROBOT2, a.r1, dr2, dr1);
  for (int u = 0; u < L; ++u) dr1[u] = relu_back(a.r1[u], dr1[u]);
  grad_linear(P, G, N, ROBOT0, a.rv, dr1, nullptr);
}

// The whole batch, serially (the host build; the kernel of ebc_sail_grad.h walks the same chains): robot [E][9],
// ob [E][R][5], n_rows [E] or null = N, target [E][2], sample_mask [E] or null -> grad [packed_floats(N)], loss_sum,
// count, action [E][2] or null (ebc_sail_forward's bytes)
inline void grad_batch(const float *P, int N, int E, int R, const double *robot, const double *ob, const long long *n_rows,
                       const double *target, const unsigned char *sample_mask, float grad_scale, float *grad, double *loss_sum,
                       long long *count, double *action) {
  const size_t PF = packed_floats(N);
  std::vector<double> total(PF, 0.0);
  std::vector<float> G(PF);
  std::vector<GradActs> acts(1);
  double loss = 0.0;
  long long live_envs = 0;
  for (int c0 = 0; c0 < E; c0 += EBC_SAIL_GRAD_CHUNK) {
    const int c1 = c0 + EBC_SAIL_GRAD_CHUNK < E ? c0 + EBC_SAIL_GRAD_CHUNK : E;
    for (size_t i = 0; i < PF; ++i) G[i] = 0.0f;
    double chunk_loss = 0.0;
    for (int e = c0; e < c1; ++e) {
      const double *rb = robot + (size_t)e * 9;
      const long long nr = n_rows ? n_rows[e] : (long long)N;
      GradActs &a = acts[0];
      grad_forward_env(P, N, rb, ob + (size_t)e * R * 5, a);
      if (action) {
        const bool rows_ok = nr == (long long)N, is_arrived = arrived(rb);
        action[(size_t)e * 2] = action_of(a.planned[0], is_arrived, rows_ok);
        action[(size_t)e * 2 + 1] = action_of(a.planned[1], is_arrived, rows_ok);
      }
      if (!grad_live(rb, nr, N, !sample_mask || sample_mask[e] != 0)) continue;
      const float d0 = grad_diff(a.planned[0], target[(size_t)e * 2]), d1 = grad_diff(a.planned[1], target[(size_t)e * 2 + 1]);
      const float seed[2] = {grad_scale * d0, grad_scale * d1};
      chunk_loss = chunk_loss + grad_loss(d0, d1);
      live_envs += 1;
      grad_backward_env(P, G.data(), N, a, seed);
    }
    for (size_t i = 0; i < PF; ++i) total[i] = total[i] + (double)G[i];
    loss = loss + chunk_loss;
  }
  for (size_t i = 0; i < PF; ++i) grad[i] = (float)total[i];
  *loss_sum = loss;
  *count = live_envs;
}

}  // namespace ebc_sail
