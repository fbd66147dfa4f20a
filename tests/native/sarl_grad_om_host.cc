// Host build of the product's SARL gradient rule (eb-cadrl_amd/csrc/ebc_sarl_grad_rule.h) on the WIDE rows of OM-SARL
// (the occupancy map behind the rotated columns): the same source the gradient kernel compiles, applied serially, so
// tests/test_om_train_cpu.py can hold it against torch's autograd without a GPU and tests/test_om_train_gpu.py can hold
// the kernel on ebc_sarl_net_create_om's networks against it byte for byte.  tests/native/sarl_grad_host.cc stays the
// build of the plain rows; with om_width = 0 the two give the same bytes.
//
// widths[12] here: the ROTATED width T, then the units of mlp1 (2), mlp2 (2), attention (3), mlp3 (4); the rows are
// T + om_width wide, as ebc_sarl_net_create_om takes them.
//
// Built as a shared library (the sarl_grad_om_host* functions below) and as a program of its own:
//   sarl_grad_om_host IN OUT   IN:  int32 count, then per batch int32 widths[12], self_dim, global, B, R, has_n_valid,
//                                   has_mask, om_width; float32 grad_scale; float32 P[packed floats]; float32
//                                   rows[B*R*(widths[0]+om_width)]; int64 n_valid[B] when has_n_valid; float32 target[B];
//                                   uint8 mask[B] when has_mask
//                              OUT: per batch float32 grad[packed floats]; float64 loss_sum; int64 count; float32 value[B];
//                                   float32 attention[B*R]
// which is what the sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>

#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_sarl_grad_rule.h"

namespace {

ebc_sarl::GradDims wide_dims(const int *widths, int self_dim, int global, int om_width) {
  int w[EBC_SARL_GRAD_LAYERS + 1];
  for (int i = 0; i <= EBC_SARL_GRAD_LAYERS; ++i) w[i] = widths[i];
  w[0] += om_width;
  return ebc_sarl::grad_dims(w, self_dim, global);
}

template <typename T>
bool read_n(FILE *f, std::vector<T> &out, size_t n) {
  out.resize(n);
  return n == 0 || fread(out.data(), sizeof(T), n, f) == n;
}

}  // namespace

extern "C" int sarl_grad_om_host_max_om() { return EBC_SARL_GRAD_MAX_OM; }
extern "C" int sarl_grad_om_host_max_wide() { return EBC_SARL_GRAD_MAX_WIDE; }
extern "C" int sarl_grad_om_host_max_row() { return EBC_SARL_GRAD_MAX_ROW; }
extern "C" int sarl_grad_om_host_refused(const int *widths, int self_dim, int om_width) {
  return ebc_sarl::grad_dims_refused_wide(widths, self_dim, om_width);
}
extern "C" long long sarl_grad_om_host_floats(const int *widths, int self_dim, int global, int om_width) {
  return (long long)wide_dims(widths, self_dim, global, om_width).floats;
}
extern "C" void sarl_grad_om_host_pack(const int *widths, int self_dim, int global, int om_width, const float *const *weight,
                                       const float *const *bias, float *P) {
  ebc_sarl::grad_pack(wide_dims(widths, self_dim, global, om_width), weight, bias, P);
}
extern "C" void sarl_grad_om_host(const int *widths, int self_dim, int global, int om_width, const float *P, int B, int R, const float *rows,
                                  const long long *n_valid, const float *target, const unsigned char *mask, float grad_scale, float *grad,
                                  double *loss_sum, long long *count, float *value, float *attention) {
  ebc_sarl::grad_batch(P, wide_dims(widths, self_dim, global, om_width), B, R, rows, n_valid, target, mask, grad_scale, grad, loss_sum, count,
                       value, attention);
}

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
    int head[19];
    float grad_scale;
    if (fread(head, sizeof(int), 19, in) != 19 || fread(&grad_scale, sizeof(float), 1, in) != 1 ||
        ebc_sarl::grad_dims_refused_wide(head, head[12], head[18]) || head[14] < 0 || head[15] < 1 || head[15] > 1024) {
      rc = 1;
      break;
    }
    const ebc_sarl::GradDims D = wide_dims(head, head[12], head[13], head[18]);
    const size_t B = head[14], R = head[15];
    std::vector<float> P, rows, target;
    std::vector<long long> n_valid;
    std::vector<unsigned char> mask;
    if (!read_n(in, P, D.floats) || !read_n(in, rows, B * R * D.T) || (head[16] && !read_n(in, n_valid, B)) || !read_n(in, target, B) ||
        (head[17] && !read_n(in, mask, B))) {
      rc = 1;
      break;
    }
    std::vector<float> grad(D.floats), value(B), attention(B * R);
    double loss = 0.0;
    long long count = 0;
    ebc_sarl::grad_batch(P.data(), D, (int)B, (int)R, rows.data(), head[16] ? n_valid.data() : nullptr, target.data(),
                         head[17] ? mask.data() : nullptr, grad_scale, grad.data(), &loss, &count, value.data(), attention.data());
    if (fwrite(grad.data(), sizeof(float), grad.size(), out) != grad.size() || fwrite(&loss, sizeof(double), 1, out) != 1 ||
        fwrite(&count, sizeof(long long), 1, out) != 1 || fwrite(value.data(), sizeof(float), B, out) != B ||
        fwrite(attention.data(), sizeof(float), B * R, out) != B * R)
      rc = 1;
  }
  fclose(in);
  if (fclose(out) != 0) rc = 1;
  if (rc) fprintf(stderr, "malformed input or short write\n");
  else printf("sarl_grad_om_host: %d batches\n", batches);
  return rc;
}
