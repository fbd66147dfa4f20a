// ebc_cadrl_rule.h — the scalar rule of a CADRL decision (rl/policy/cadrl.py:194-217), ONE definition for the kernel
// (hipcc, ebc_cadrl.h) and for the host build the tests compare it with (g++, tests/native/cadrl_host.cc).
//
//   m      = torch.min over the rows of one (env, action): a NaN among them makes the result NaN (fminf would drop it)
//   value  = reward + discount * (double)m: two rounded float64 operations (both builds compile with
//            -ffp-contract=off); every NaN result is the one quiet NaN below, so the builds agree byte for byte
//   choice = the reference's running `max_min_value = -inf; if value > max_min_value`: the first maximum wins, a NaN
//            is never better, and no value above -inf leaves the choice at -1
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EBC_CADRL_HD __host__ __device__ inline
#else
#define EBC_CADRL_HD inline
#endif

#define EBC_CADRL_MAX_ACTIONS 128
#define EBC_CADRL_MAX_ROWS 128

namespace ebc_cadrl {

EBC_CADRL_HD float nan_f32() {
  const uint32_t u = 0x7fc00000u;
  float x;
  memcpy(&x, &u, 4);
  return x;
}
EBC_CADRL_HD double nan_f64() {
  const uint64_t u = 0x7ff8000000000000ull;
  double x;
  memcpy(&x, &u, 8);
  return x;
}
EBC_CADRL_HD double neg_inf() {
  const uint64_t u = 0xfff0000000000000ull;
  double x;
  memcpy(&x, &u, 8);
  return x;
}

// the rows an env holds: n_valid clamped to [0, R]
EBC_CADRL_HD int clamp_rows(long long v, int R) { return v < 0 ? 0 : (v > R ? R : (int)v); }

// one step of the NaN-propagating minimum: m once NaN stays NaN (both comparisons are false), a NaN x replaces m
EBC_CADRL_HD float min_step(float m, float x) { return (x < m || x != x) ? x : m; }

// the minimum of v[0 .. n) (elements `stride` apart); no row gives NaN
EBC_CADRL_HD float min_rows(const float *v, int n, int stride) {
  if (n <= 0) return nan_f32();
  float m = v[0];
  for (int r = 1; r < n; ++r) m = min_step(m, v[(size_t)r * stride]);
  return m;
}

EBC_CADRL_HD double action_value(double reward, double discount, float m) {
  const double scaled = discount * (double)m;
  const double value = reward + scaled;
  return value != value ? nan_f64() : value;
}

// `if min_value > max_min_value`: false for a NaN on either side
EBC_CADRL_HD bool better(double value, double best) { return value > best; }

}  // namespace ebc_cadrl
