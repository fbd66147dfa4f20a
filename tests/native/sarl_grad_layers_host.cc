// Host build of the product's SARL gradient rule (eb-cadrl_amd/csrc/ebc_sarl_grad_rule.h) with the WIDE buffers: the same
// source and the same serial loops as tests/native/sarl_grad_host.cc, their per-row stride raised from 256 to 640
// (EBC_SARL_GRAD_HOST_WIDTH), so that it holds the networks of the layer form of the gradient kernel
// (ebc_sarl_net_create_layers: hidden layers up to 640).  The stride moves no byte of any result:
// tests/test_sarl_grad_layers_cpu.py holds this build to sarl_grad_host.cc's bytes on the narrow networks and to torch's
// autograd on the wide ones, and tests/test_sarl_grad_layers_gpu.py holds the layer form's kernels to it byte for byte.
//
// widths[12]: the ROTATED width T, then the units of mlp1 (2), mlp2 (2), attention (3), mlp3 (4); the rows are
// T + om_width wide, as ebc_sarl_net_create_layers takes them.
//
// Built as a shared library (the sarl_grad_layers_host* functions below) and as a program of its own:
//   sarl_grad_layers_host IN OUT   the files of tests/native/sarl_grad_om_host.cc: per batch int32 widths[12], self_dim,
//                                  global, B, R, has_n_valid, has_mask, om_width; float32 grad_scale; P; rows; n_valid;
//                                  target; mask -> grad; float64 loss_sum; int64 count; value; attention
// which is what the sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>

#include <vector>

#define EBC_SARL_GRAD_HOST_WIDTH 640
#include "../../eb-cadrl_amd/csrc/ebc_sarl_grad_rule.h"

static_assert(EBC_SARL_GRAD_HOST_WIDTH >= EBC_SARL_GRAD_LAYERS_MAX_WIDTH, "the wide build holds the layer form's widest layer");

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

extern "C" int sarl_grad_layers_host_max_width() { return EBC_SARL_GRAD_LAYERS_MAX_WIDTH; }
extern "C" int sarl_grad_layers_host_max_rows() { return EBC_SARL_GRAD_LAYERS_MAX_ROWS; }
extern "C" int sarl_grad_layers_host_run_slots() { return EBC_SARL_GRAD_LAYERS_RUN_SLOTS; }
extern "C" int sarl_grad_layers_host_stride() { return EBC_SARL_GRAD_HOST_WIDTH; }
extern "C" int sarl_grad_layers_host_chunk() { return EBC_SARL_GRAD_CHUNK; }
extern "C" int sarl_grad_layers_host_refused(const int *widths, int self_dim, int om_width) {
  return ebc_sarl::grad_dims_refused_layers(widths, self_dim, om_width);
}
// the chunk form's limits, from the same header: unchanged by the layer form
extern "C" int sarl_grad_layers_host_refused_chunk(const int *widths, int self_dim, int om_width) {
  return ebc_sarl::grad_dims_refused_wide(widths, self_dim, om_width);
}
extern "C" long long sarl_grad_layers_host_floats(const int *widths, int self_dim, int global, int om_width) {
  return (long long)wide_dims(widths, self_dim, global, om_width).floats;
}
extern "C" void sarl_grad_layers_host_layer(const int *widths, int self_dim, int global, int om_width, int l, long long *at, int *inputs,
                                            int *padded) {
  const ebc_sarl::GradDims D = wide_dims(widths, self_dim, global, om_width);
  *at = (long long)D.at[l];
  *inputs = D.K[l];
  *padded = D.Op[l];
}
extern "C" void sarl_grad_layers_host_pack(const int *widths, int self_dim, int global, int om_width, const float *const *weight,
                                           const float *const *bias, float *P) {
  ebc_sarl::grad_pack(wide_dims(widths, self_dim, global, om_width), weight, bias, P);
}
extern "C" void sarl_grad_layers_host(const int *widths, int self_dim, int global, int om_width, const float *P, int B, int R, const float *rows,
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
        ebc_sarl::grad_dims_refused_layers(head, head[12], head[18]) || head[14] < 0 || head[15] < 1 || head[15] > 1024) {
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
  else printf("sarl_grad_layers_host: %d batches\n", batches);
  return rc;
}
