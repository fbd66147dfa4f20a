// ebc_dagger.h — the kernels of ebc_sail_dagger_k (include/ebcsim.h): a closed-loop rollout in which the SAIL network
// drives while the ORCA robot labels every state the network visits (DAgger: Ross, Gordon and Bagnell, AISTATS 2011).
//
// Per step the entry enqueues four launches on the handle's stream:
//   1 dagger_label_kernel   records robot[k], ob[k], n_rows[k] of the current state and writes expert_action[k]
//   2 sail_kernel           (ebcsim_sail.hip) reads those records in place -> learner_action[k]
//   3 dagger_select_kernel  robot_action_out[k] = take_expert[k] ? expert_action[k] : learner_action[k], as bits
//   4 the step              (ebc_step) reads robot_action_out[k]
// The gathers have to precede the network (it reads them) and the select follows both actions, so neither can move into
// the other's launch without touching sail_kernel or the step kernels; the label kernel is where the copy of the robot
// state, observe_kernel, row_counts_kernel and orca_robot_kernel of the composition become one read of the state.
#pragma once

#include "ebc_kernels.h"

namespace ebc {

// Lane layout of orca_robot_kernel: one GS-lane group per env, lane j = row j of the observation, GS >= N + S.
//   lane j < N + S writes ob[e][j][0 .. 5): ebc_observe's row (zeros where the env has no such row)
//   lane 0 of the group writes robot[e][0 .. 9) (the bytes of the state, as ebc_get_state copies them), n_rows[e]
//   (ebc_row_counts) and, after the solve, expert[e][0 .. 2) (ebc_robot_orca)
// The records leave from the registers the solve was fed from.  Their stores are issued by orca_robot_solve's hook: after
// the last global load has been consumed and before the solve, which waits on LDS only, so no s_waitcnt of the solve
// stands behind them.  LDS: OrcaLds<GS> and nothing else.
template <int GS>
__global__ __launch_bounds__(EBC_WAVE) void dagger_label_kernel(EbcParams p, DevState s, double safety_space, RobotSim sim,
                                                                 double *robot_out, double *ob_out, long long *rows_out,
                                                                 double *expert) {
  __shared__ __align__(16) unsigned char scratch[OrcaLds<GS>::BYTES];
  const RobotLane l = robot_lane<GS>(s);
  const int R = s.N + s.S;
  const ObsRow row = obs_row(env_rows(s, l.ee), l.j, l.n, l.ns);
  double rb[9];
  const double *src = s.robot + l.ee * 9;
#pragma unroll
  for (int c = 0; c < 9; ++c) rb[c] = src[c];
  float ox, oy;
  orca_robot_solve<GS>(p, s, safety_space, sim, scratch, l, rb, row, ox, oy, [&]() {
    if (l.e_ok && l.j < R) {
      double *o = ob_out + (l.ee * R + l.j) * 5;
      o[0] = row.px; o[1] = row.py; o[2] = row.vx; o[3] = row.vy; o[4] = row.radius;
    }
    if (l.e_ok && l.j == 0) {
      double *r = robot_out + l.ee * 9;
#pragma unroll
      for (int c = 0; c < 9; ++c) r[c] = rb[c];
      rows_out[l.ee] = (long long)l.n + l.ns;
    }
  });
  if (l.e_ok && l.j == 0) {
    expert[2 * l.ee] = (double)ox;  // getAgentVelocity -> Python float
    expert[2 * l.ee + 1] = (double)oy;
  }
}

// robot_action_out[e] = take[e] ? expert[e] : learner[e]: 64-bit words chosen, never arithmetic (a NaN of the side not
// taken reaches nothing, and a NaN taken keeps its payload).  take == nullptr: the learner always acts.  Thread = one
// of the E * 2 words.
__global__ __launch_bounds__(256) void dagger_select_kernel(int E, const uint8_t *take, const unsigned long long *learner,
                                                            const unsigned long long *expert, unsigned long long *out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * E) return;
  const bool t = take && take[g >> 1] != 0;
  out[g] = t ? expert[g] : learner[g];
}

}  // namespace ebc
