// Host build of the product's SAIL gradient rule (eb-cadrl_amd/csrc/ebc_sail_grad_rule.h) for the tests: the same source
// the kernel compiles, applied serially, so tests/test_sail_train_cpu.py can hold it against torch's autograd without a
// GPU and tests/test_sail_train_gpu.py can hold the kernel against it byte for byte.
//
// Built as a shared library (the sail_grad_host_* functions below) and as a program of its own:
//   sail_grad_host [N [E]]     a seeded batch with masked, arrived and ragged envs that carry NaN; prints the loss, the
//                              count and a checksum of the gradient's bytes
// which is what a sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_sail_grad_rule.h"

extern "C" int sail_grad_host_chunk() { return EBC_SAIL_GRAD_CHUNK; }
extern "C" int sail_grad_host_group(int N) { return ebc_sail::grad_group_envs(N); }
extern "C" long long sail_grad_host_packed_floats(int N) { return (long long)ebc_sail::packed_floats(N); }

// weight / bias: 14 pointers in torch's layout -> the packed image P [packed_floats(N)]
extern "C" void sail_grad_host_pack(int N, const float *const *weight, const float *const *bias, float *P) { ebc_sail::pack(N, weight, bias, P); }

// P: the packed image; robot [E][9]; ob [E][R][5]; n_rows [E] or NULL; target [E][2]; mask [E] or NULL
// -> grad [packed_floats(N)], loss_sum, count, action [E][2] or NULL
extern "C" void sail_grad_host(int N, const float *P, const double *robot, const double *ob, const long long *n_rows, const double *target,
                               const unsigned char *mask, float grad_scale, int E, int R, float *grad, double *loss_sum, long long *count,
                               double *action) {
  ebc_sail::grad_batch(P, N, E, R, robot, ob, n_rows, target, mask, grad_scale, grad, loss_sum, count, action);
}

int main(int argc, char **argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 5, E = argc > 2 ? atoi(argv[2]) : 2 * EBC_SAIL_GRAD_CHUNK + 3, R = N + 2;
  if (N < EBC_SAIL_MIN_ADULTS || N > EBC_SAIL_MAX_ADULTS || E < 0 || E > 4096) {
    fprintf(stderr, "usage: %s [N in 2..32 [E in 0..4096]]\n", argv[0]);
    return 2;
  }
  unsigned long long state = 88172645463325252ull;
  auto uniform = [&state](double lo, double hi) {  // xorshift64
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return lo + (hi - lo) * (double)(state >> 11) / 9007199254740992.0;
  };
  const size_t PF = ebc_sail::packed_floats(N);
  std::vector<float> P(PF, 0.0f);
  for (int l = 0; l < EBC_SAIL_LAYERS; ++l) {
    const int K = ebc_sail::layer_in(l, N), O = ebc_sail::layer_out(l);
    float *W = P.data() + ebc_sail::layer_offset(l, N);
    for (int k = 0; k <= K; ++k)
      for (int o = 0; o < O; ++o) W[(size_t)k * EBC_SAIL_HIDDEN + o] = (float)uniform(-0.3, 0.3);
  }
  std::vector<double> robot((size_t)E * 9), ob((size_t)E * R * 5), target((size_t)E * 2), action((size_t)E * 2);
  std::vector<long long> n_rows(E, N);
  std::vector<unsigned char> mask(E, 1);
  for (double &v : robot) v = uniform(-4, 4);
  for (double &v : ob) v = uniform(-4, 4);
  for (double &v : target) v = uniform(-1, 1);
  const double nan = (double)ebc_lstm::float_of(0x7fc00000u);
  for (int e = 0; e < E; ++e) {
    robot[(size_t)e * 9 + 4] = 0.3;
    for (int r = N; r < R; ++r) ob[((size_t)e * R + r) * 5] = nan;
    if (e % 5 == 1) mask[e] = 0, robot[(size_t)e * 9 + 2] = nan, target[(size_t)e * 2] = nan;
    if (e % 7 == 2) n_rows[e] = N - 1, ob[(size_t)e * R * 5 + 1] = nan;
    if (e % 9 == 3) robot[(size_t)e * 9 + 5] = robot[(size_t)e * 9] + 0.1, robot[(size_t)e * 9 + 6] = robot[(size_t)e * 9 + 1];
  }
  std::vector<float> grad(PF, -7.0f);
  double loss = -1.0;
  long long count = -1;
  sail_grad_host(N, P.data(), robot.data(), ob.data(), n_rows.data(), target.data(), mask.data(), 0.125f, E, R, grad.data(), &loss, &count,
                 action.data());
  unsigned long long sum = 1469598103934665603ull;
  bool finite = loss == loss;
  for (size_t i = 0; i < PF; ++i) {
    sum = (sum ^ ebc_lstm::bits_of(grad[i])) * 1099511628211ull;
    finite = finite && grad[i] == grad[i] && grad[i] - grad[i] == 0.0f;
  }
  printf("sail_grad_host: N %d E %d loss %.17g count %lld checksum %016llx finite %d\n", N, E, loss, count, sum, (int)finite);
  return finite ? 0 : 1;
}
