// ebc_cadrl.h — the reduction and the decision of rl/policy/cadrl.py:194-217 as one kernel: the value network's one
// output per (robot, other) row in, per action the minimum over the env's rows and reward + discount * min, per env the
// reference's choice.  The arithmetic is ebc_cadrl_rule.h.
//
// One wave per env.  The env's actions go through LDS 64 at a time: the wave reads the A' * R floats of 64 actions
// with consecutive lanes on consecutive addresses and leaves row r of action a at s[a * (R | 1) + r]; lane a then
// walks its own action's rows (the odd stride keeps the 32 lanes of a half wave on 32 banks).  Rows at or past the
// env's count are neither loaded nor read.  Lane a holds the values of actions a and a + 64; the choice is a wave
// maximum over the lanes' better value and a ballot for the lowest lane that holds it, the first half of the actions
// asked before the second: the lowest index among equal values, as the serial rule gives.  No atomics, no polling.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_cadrl_rule.h"

namespace ebc {

struct CadrlLaunch {
  const float *v;            // [E][A][R]
  const long long *n_valid;  // [E] or nullptr = R
  const double *reward;      // [E][A]
  double *values;            // [E][A]
  int *choice;               // [E]
  double discount;
  int A, R;
};

__global__ __launch_bounds__(64) void cadrl_decide_kernel(const CadrlLaunch a) {
  extern __shared__ float cadrl_lds[];  // 64 * (R | 1) floats
  const int lane = threadIdx.x, A = a.A, R = a.R, RS = R | 1;
  const size_t e = blockIdx.x;
  const int n = ebc_cadrl::clamp_rows(a.n_valid ? a.n_valid[e] : (long long)R, R);
  const float *v = a.v + e * A * R;
  const double *reward = a.reward + e * A;
  double *values = a.values + e * A;
  double key[2];  // the lane's two values as the rule ranks them: a NaN, or no action, counts as -inf
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a0 = 64 * h, na = A - a0 < 64 ? A - a0 : 64;  // wave-uniform
    key[h] = ebc_cadrl::neg_inf();
    if (na <= 0) continue;
    if (h) __syncthreads();  // the first half's rows have been read
    for (int i = lane; i < na * R; i += 64) {
      const int aa = i / R, r = i - aa * R;
      if (r < n) cadrl_lds[aa * RS + r] = v[(size_t)a0 * R + i];
    }
    __syncthreads();
    if (lane < na) {
      const float m = ebc_cadrl::min_rows(cadrl_lds + lane * RS, n, 1);
      const double value = ebc_cadrl::action_value(reward[a0 + lane], a.discount, m);
      values[a0 + lane] = value;
      if (ebc_cadrl::better(value, key[h])) key[h] = value;
    }
  }
  const double mine = ebc_cadrl::better(key[1], key[0]) ? key[1] : key[0];
  double best = mine;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(best, o, 64);
    best = ebc_cadrl::better(other, best) ? other : best;
  }
  int choice = -1;
  if (ebc_cadrl::better(best, ebc_cadrl::neg_inf())) {
    const unsigned long long first = __ballot(key[0] == best), second = __ballot(key[1] == best);
    choice = first ? __builtin_ctzll(first) : 64 + __builtin_ctzll(second);
  }
  if (lane == 0) a.choice[e] = choice;
}

}  // namespace ebc
