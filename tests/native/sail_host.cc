// Host build of the product's SAIL arithmetic (eb-cadrl_amd/csrc/ebc_sail_rule.h) for the tests: the same source the
// kernel compiles, applied serially per env, so tests/test_sail_cpu.py can hold it against torch and the reference's
// recorded run without a GPU and tests/test_sail_gpu.py can hold the kernel against it byte for byte.
//
// Built as a shared library (sail_host below) and as a program of its own:
//   sail_host IN OUT     IN:  int32 count, then per batch int32 N, E, R, has_n_rows; per layer of ebc_sail::Layer float32
//                             weight[out * in] then bias[out]; float64 robot[E*9]; float64 ob[E*R*5]; int64 n_rows[E] when
//                             has_n_rows
//                        OUT: per batch float64 action[E*2]; float32 feat_joint[E*64]
// which is what the sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>

#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_sail_rule.h"

// weight / bias: 14 pointers in torch's layout; robot [E][9]; ob [E][R][5]; n_rows [E] int64 or NULL = N;
// -> action [E][2], feat_joint [E][64] or NULL
extern "C" void sail_host(int N, const float *const *weight, const float *const *bias, const double *robot, const double *ob,
                          const long long *n_rows, int E, int R, double *action, float *feat_joint) {
  std::vector<float> P(ebc_sail::packed_floats(N));
  ebc_sail::pack(N, weight, bias, P.data());
  for (int e = 0; e < E; ++e)
    ebc_sail::forward_env(P.data(), N, robot + (size_t)e * 9, ob + (size_t)e * R * 5, n_rows ? n_rows[e] : (long long)N,
                          action + (size_t)e * 2, feat_joint ? feat_joint + (size_t)e * EBC_SAIL_HIDDEN : nullptr);
}

// envs per workgroup of the kernel at this adult_num
extern "C" int sail_host_group(int N) { return ebc_sail::group_envs(N); }

namespace {

template <typename T>
bool read_n(FILE *f, std::vector<T> &out, size_t n) {
  out.resize(n);
  return n == 0 || fread(out.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE *in = fopen(argv[1], "rb"), *out = in ? fopen(argv[2], "wb") : nullptr;
  if (!in || !out) {
    fprintf(stderr, "cannot open %s\n", in ? argv[2] : argv[1]);
    if (in) fclose(in);
    return 2;
  }
  int rc = 0, count = 0;
  if (fread(&count, sizeof(int), 1, in) != 1) rc = 1;
  for (int b = 0; !rc && b < count; ++b) {
    int head[4];
    if (fread(head, sizeof(int), 4, in) != 4 || head[0] < EBC_SAIL_MIN_ADULTS || head[0] > EBC_SAIL_MAX_ADULTS || head[1] < 0 ||
        head[1] > (1 << 20) || head[2] < head[0] || head[2] > 1024) {
      rc = 1;
      break;
    }
    const int N = head[0];
    const size_t E = head[1], R = head[2];
    std::vector<float> w[EBC_SAIL_LAYERS], bs[EBC_SAIL_LAYERS];
    const float *wp[EBC_SAIL_LAYERS], *bp[EBC_SAIL_LAYERS];
    for (int l = 0; !rc && l < EBC_SAIL_LAYERS; ++l) {
      if (!read_n(in, w[l], (size_t)ebc_sail::layer_in(l, N) * ebc_sail::layer_out(l)) || !read_n(in, bs[l], ebc_sail::layer_out(l))) rc = 1;
      wp[l] = w[l].data();
      bp[l] = bs[l].data();
    }
    std::vector<double> robot, ob;
    std::vector<long long> n_rows;
    if (rc || !read_n(in, robot, E * 9) || !read_n(in, ob, E * R * 5) || (head[3] && !read_n(in, n_rows, E))) {
      rc = 1;
      break;
    }
    std::vector<double> action(E * 2);
    std::vector<float> feat(E * EBC_SAIL_HIDDEN);
    sail_host(N, wp, bp, robot.data(), ob.data(), head[3] ? n_rows.data() : nullptr, (int)E, (int)R, action.data(), feat.data());
    if (fwrite(action.data(), sizeof(double), E * 2, out) != E * 2 || fwrite(feat.data(), sizeof(float), E * EBC_SAIL_HIDDEN, out) != E * EBC_SAIL_HIDDEN)
      rc = 1;
  }
  fclose(in);
  if (fclose(out) != 0) rc = 1;
  if (rc) fprintf(stderr, "malformed input or short write\n");
  else printf("sail_host: %d batches\n", count);
  return rc;
}
