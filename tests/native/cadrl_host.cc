// Host build of the product's CADRL decision rule (eb-cadrl_amd/csrc/ebc_cadrl_rule.h) for the tests: the same source
// the decision kernel compiles, applied serially per env, so tests/test_cadrl_cpu.py can hold it against torch.min and
// the reference's running choice without a GPU and tests/test_cadrl_gpu.py can hold the kernel against it byte for byte.
//
// Built as a shared library (cadrl_host below) and as a program of its own:
//   cadrl_host IN OUT    IN:  int32 count, then per batch int32 E, A, R, has_n_valid; float64 discount; float32 v[E*A*R];
//                             int64 n_valid[E] when has_n_valid; float64 reward[E*A]
//                        OUT: per batch float64 values[E*A]; int32 choice[E]
// which is what the sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>

#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_cadrl_rule.h"

// v [E][A][R]; n_valid [E] int64 or NULL = R (above R counts as R, below 0 as 0); reward [E][A] -> values [E][A], choice [E]
extern "C" void cadrl_host(const float *v, const long long *n_valid, const double *reward, double discount, int E, int A,
                           int R, double *values, int *choice) {
  for (int e = 0; e < E; ++e) {
    const int n = ebc_cadrl::clamp_rows(n_valid ? n_valid[e] : (long long)R, R);
    double best = ebc_cadrl::neg_inf();
    int pick = -1;
    for (int a = 0; a < A; ++a) {
      const size_t at = (size_t)e * A + a;
      const float m = ebc_cadrl::min_rows(v + at * R, n, 1);
      const double value = ebc_cadrl::action_value(reward[at], discount, m);
      values[at] = value;
      if (ebc_cadrl::better(value, best)) {
        best = value;
        pick = a;
      }
    }
    choice[e] = pick;
  }
}

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
    double discount;
    if (fread(head, sizeof(int), 4, in) != 4 || fread(&discount, sizeof(double), 1, in) != 1 || head[0] < 0 || head[1] < 1 ||
        head[2] < 1 || head[1] > EBC_CADRL_MAX_ACTIONS || head[2] > EBC_CADRL_MAX_ROWS) {
      rc = 1;
      break;
    }
    const size_t E = head[0], A = head[1], R = head[2];
    std::vector<float> v;
    std::vector<long long> n_valid;
    std::vector<double> reward;
    if (!read_n(in, v, E * A * R) || (head[3] && !read_n(in, n_valid, E)) || !read_n(in, reward, E * A)) {
      rc = 1;
      break;
    }
    std::vector<double> values(E * A);
    std::vector<int> choice(E);
    cadrl_host(v.data(), head[3] ? n_valid.data() : nullptr, reward.data(), discount, (int)E, (int)A, (int)R, values.data(),
               choice.data());
    if (fwrite(values.data(), sizeof(double), E * A, out) != E * A || fwrite(choice.data(), sizeof(int), E, out) != E) rc = 1;
  }
  fclose(in);
  if (fclose(out) != 0) rc = 1;
  if (rc) fprintf(stderr, "malformed input or short write\n");
  else printf("cadrl_host: %d batches\n", count);
  return rc;
}
