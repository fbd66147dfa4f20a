// Host build of the product's CADRL gradient rule (eb-cadrl_amd/csrc/ebc_cadrl_grad_rule.h) for the tests: the same source
// the gradient kernel compiles, applied serially, so tests/test_cadrl_train_cpu.py can hold it against torch's autograd
// without a GPU and tests/test_cadrl_train_gpu.py can hold the kernel against it byte for byte.
//
// Built as a shared library (the cadrl_grad_host* functions below) and as a program of its own:
//   cadrl_grad_host IN OUT   IN:  int32 count, then per batch int32 widths[5], B, R, has_n_valid, has_mask; float32
//                                 grad_scale; float32 P[packed floats]; float32 rows[B*R*widths[0]]; int64 n_valid[B] when
//                                 has_n_valid; float32 target[B]; uint8 mask[B] when has_mask
//                            OUT: per batch float32 grad[packed floats]; float64 loss_sum; int64 count; float32 value[B];
//                                 int32 min_row[B]
// which is what the sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>

#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_cadrl_grad_rule.h"

extern "C" int cadrl_grad_host_chunk() { return EBC_CADRL_GRAD_CHUNK; }
extern "C" int cadrl_grad_host_refused(const int *widths) { return ebc_cadrl::grad_dims_refused(widths); }
extern "C" long long cadrl_grad_host_floats(const int *widths) { return (long long)ebc_cadrl::grad_dims(widths).floats; }
// layer l's offset in the packed image and its padded width
extern "C" void cadrl_grad_host_layer(const int *widths, int l, long long *at, int *padded) {
  const ebc_cadrl::GradDims D = ebc_cadrl::grad_dims(widths);
  *at = (long long)D.at[l];
  *padded = D.Op[l];
}
extern "C" void cadrl_grad_host_pack(const int *widths, const float *const *weight, const float *const *bias, float *P) {
  ebc_cadrl::grad_pack(ebc_cadrl::grad_dims(widths), weight, bias, P);
}
extern "C" void cadrl_grad_host(const int *widths, const float *P, int B, int R, const float *rows, const long long *n_valid,
                                const float *target, const unsigned char *mask, float grad_scale, float *grad, double *loss_sum,
                                long long *count, float *value, int *min_row) {
  ebc_cadrl::grad_batch(P, ebc_cadrl::grad_dims(widths), B, R, rows, n_valid, target, mask, grad_scale, grad, loss_sum, count, value,
                        min_row);
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
  int rc = 0, batches = 0;
  if (fread(&batches, sizeof(int), 1, in) != 1) rc = 1;
  for (int i = 0; !rc && i < batches; ++i) {
    int head[9];
    float grad_scale;
    if (fread(head, sizeof(int), 9, in) != 9 || fread(&grad_scale, sizeof(float), 1, in) != 1 || ebc_cadrl::grad_dims_refused(head) ||
        head[5] < 0 || head[6] < 1 || head[6] > EBC_CADRL_MAX_ROWS) {
      rc = 1;
      break;
    }
    const ebc_cadrl::GradDims D = ebc_cadrl::grad_dims(head);
    const size_t B = head[5], R = head[6];
    std::vector<float> P, rows, target;
    std::vector<long long> n_valid;
    std::vector<unsigned char> mask;
    if (!read_n(in, P, D.floats) || !read_n(in, rows, B * R * D.K[0]) || (head[7] && !read_n(in, n_valid, B)) || !read_n(in, target, B) ||
        (head[8] && !read_n(in, mask, B))) {
      rc = 1;
      break;
    }
    std::vector<float> grad(D.floats), value(B);
    std::vector<int> min_row(B);
    double loss = 0.0;
    long long count = 0;
    ebc_cadrl::grad_batch(P.data(), D, (int)B, (int)R, rows.data(), head[7] ? n_valid.data() : nullptr, target.data(),
                          head[8] ? mask.data() : nullptr, grad_scale, grad.data(), &loss, &count, value.data(), min_row.data());
    if (fwrite(grad.data(), sizeof(float), grad.size(), out) != grad.size() || fwrite(&loss, sizeof(double), 1, out) != 1 ||
        fwrite(&count, sizeof(long long), 1, out) != 1 || fwrite(value.data(), sizeof(float), B, out) != B ||
        fwrite(min_row.data(), sizeof(int), B, out) != B)
      rc = 1;
  }
  fclose(in);
  if (fclose(out) != 0) rc = 1;
  if (rc) fprintf(stderr, "malformed input or short write\n");
  else printf("cadrl_grad_host: %d batches\n", batches);
  return rc;
}
