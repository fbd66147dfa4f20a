// ebcsim_cadrl_grad.hip — training the CADRL value network: the network object ebc_cadrl_net_* (the packed image of
// ebc_cadrl_grad_rule.h in device memory, with the scratch of the chunk partials) and ebc_cadrl_grad (the fused forward +
// minimum + backward kernel and the reduction of its partials, ebc_cadrl_grad.h).  Its own translation unit: the decision's
// unit and the two-layer blocks keep their code.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_cadrl_grad.h"
#include "ebc_host.h"

namespace {

using ebc_host::fail;

constexpr int kMaxChunksPerLaunch = 1024;  // 1024 chunks of partials (114 MB at the reference widths) before the float64 sums take over

struct CadrlNet {
  int device = 0;
  ebc_cadrl::GradDims D;
  float *P = nullptr;        // the packed image
  void *scratch = nullptr;   // float64 sums | chunk losses | chunk counts | chunk partials
  size_t scratch_bytes = 0;
};

bool capturing(void *stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

}  // namespace

extern "C" int ebc_cadrl_net_create(const EbcCadrlNetWeights *weights, int device_id, void **net_out) {
  if (!weights || weights->struct_size != sizeof(EbcCadrlNetWeights)) return fail(EBC_ERR_INVALID, "EbcCadrlNetWeights.struct_size");
  if (!net_out) return fail(EBC_ERR_INVALID, "ebc_cadrl_net_create: null net_out");
  if (weights->n_layers != EBC_CADRL_GRAD_LAYERS)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_net_create: value_network has " + std::to_string(weights->n_layers) + " Linear layers, the gradient takes exactly 4");
  const int bad = ebc_cadrl::grad_dims_refused(weights->widths);
  if (bad == 1)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_net_create: rows of " + std::to_string(weights->widths[0]) + " floats, the gradient takes 1 .. " +
                                         std::to_string(EBC_CADRL_GRAD_MAX_IN));
  if (bad == EBC_CADRL_GRAD_LAYERS + 1)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_net_create: the last layer has " + std::to_string(weights->widths[4]) + " outputs, the gradient takes exactly 1");
  if (bad)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_net_create: layer " + std::to_string(bad - 1) + " has " + std::to_string(weights->widths[bad - 1]) +
                                         " units, the gradient takes 1 .. " + std::to_string(EBC_CADRL_GRAD_MAX_WIDTH));
  for (int l = 0; l < EBC_CADRL_GRAD_LAYERS; ++l)
    if (!weights->weight[l] || !weights->bias[l]) return fail(EBC_ERR_INVALID, "ebc_cadrl_net_create: null weight or bias of layer " + std::to_string(l + 1));
  HIP_TRY(hipSetDevice(device_id));
  CadrlNet *n = new CadrlNet;
  n->device = device_id;
  n->D = ebc_cadrl::grad_dims(weights->widths);
  std::vector<float> image(n->D.floats);
  ebc_cadrl::grad_pack(n->D, weights->weight, weights->bias, image.data());
  hipError_t err = hipMalloc(&n->P, image.size() * sizeof(float));
  if (err == hipSuccess) err = hipMemcpy(n->P, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (n->P) (void)hipFree(n->P);
    delete n;
    return fail(EBC_ERR_DEVICE, std::string("ebc_cadrl_net_create: ") + hipGetErrorString(err));
  }
  *net_out = n;
  return EBC_OK;
}

extern "C" int ebc_cadrl_net_destroy(void *net) {
  if (!net) return EBC_OK;
  CadrlNet *n = static_cast<CadrlNet *>(net);
  (void)hipSetDevice(n->device);
  if (n->scratch) (void)hipFree(n->scratch);
  if (n->P) (void)hipFree(n->P);
  delete n;
  return EBC_OK;
}

extern "C" int ebc_cadrl_net_packed_floats(void *net, int64_t *floats_out) {
  if (!net || !floats_out) return fail(EBC_ERR_INVALID, "ebc_cadrl_net_packed_floats: null argument");
  *floats_out = (int64_t)static_cast<CadrlNet *>(net)->D.floats;
  return EBC_OK;
}

extern "C" int ebc_cadrl_net_get_packed(void *net, void *stream, float *dst_dev) {
  if (!net || !dst_dev) return fail(EBC_ERR_INVALID, "ebc_cadrl_net_get_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_net_get_packed: the stream is being captured into a HIP graph");
  CadrlNet *n = static_cast<CadrlNet *>(net);
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipMemcpyAsync(dst_dev, n->P, (size_t)n->D.floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_cadrl_net_set_packed(void *net, void *stream, const float *src_dev) {
  if (!net || !src_dev) return fail(EBC_ERR_INVALID, "ebc_cadrl_net_set_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_net_set_packed: the stream is being captured into a HIP graph");
  CadrlNet *n = static_cast<CadrlNet *>(net);
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipMemcpyAsync(n->P, src_dev, (size_t)n->D.floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_cadrl_grad(void *net, void *stream, const EbcCadrlGradArgs *args) {
  if (!net) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcCadrlGradArgs)) return fail(EBC_ERR_INVALID, "EbcCadrlGradArgs.struct_size");
  if (!args->grad || !args->loss_sum || !args->count || args->B < 0) return fail(EBC_ERR_INVALID, "ebc_cadrl_grad: grad, loss_sum, count, B");
  if (args->B > 0 && (!args->rows || !args->target)) return fail(EBC_ERR_INVALID, "ebc_cadrl_grad: rows, target");
  CadrlNet *n = static_cast<CadrlNet *>(net);
  const ebc_cadrl::GradDims &D = n->D;
  if (args->T != D.K[0])
    return fail(EBC_ERR_INVALID, "ebc_cadrl_grad: rows are " + std::to_string(args->T) + " wide, the network takes " + std::to_string(D.K[0]));
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_grad: R < 1 row slots per state (" + std::to_string(args->R) + ")");
  if (args->R > EBC_CADRL_MAX_ROWS) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_grad: R > 128 row slots per state (" + std::to_string(args->R) + ")");
  if (capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t PF = D.floats;
  const int B = args->B;
  const long long chunks = ((long long)B + EBC_CADRL_GRAD_CHUNK - 1) / EBC_CADRL_GRAD_CHUNK;
  const int per = chunks < kMaxChunksPerLaunch ? (int)(chunks > 0 ? chunks : 1) : kMaxChunksPerLaunch;
  // scratch: float64 sums [PF + 2] | loss_part [per] | count_part [per] | partial [per][PF]
  const size_t acc_bytes = (PF + 2) * sizeof(double), part_at = acc_bytes + (size_t)per * 16;
  const size_t need = part_at + (size_t)per * PF * sizeof(float);
  if (need > n->scratch_bytes) {  // grows on demand; growing waits for the device (work that reads the old scratch may be in flight)
    HIP_TRY(hipDeviceSynchronize());
    if (n->scratch) HIP_TRY(hipFree(n->scratch));
    n->scratch = nullptr;
    n->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&n->scratch, need));
    n->scratch_bytes = need;
  }
  double *acc64 = static_cast<double *>(n->scratch);
  double *loss_part = reinterpret_cast<double *>(static_cast<char *>(n->scratch) + acc_bytes);
  long long *count_part = reinterpret_cast<long long *>(loss_part + per);
  float *partial = reinterpret_cast<float *>(static_cast<char *>(n->scratch) + part_at);

  const size_t lds = ebc::cadrl_grad_lds_floats(D, args->R) * sizeof(float);  // <= 115 KB
  static size_t raised_dev[64] = {0};
  HIP_TRY(ebc_host::raise_dynamic_lds(ebc::cadrl_grad_kernel, n->device, lds, raised_dev));
  const unsigned reduce_blocks = (unsigned)((PF + 255) / 256);
  long long done = 0;
  do {
    const int now = chunks - done < per ? (int)(chunks - done) : per;
    if (now > 0) {
      ebc::CadrlGradLaunch a;
      a.rows = args->rows;
      a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
      a.target = args->target;
      a.mask = args->sample_mask;
      a.value = args->value;
      a.min_row = args->min_row;
      a.partial = partial;
      a.loss_part = loss_part;
      a.count_part = count_part;
      a.grad_scale = args->grad_scale;
      a.B = B;
      a.R = args->R;
      a.chunk0 = (int)done;
      a.D = D;
      hipLaunchKernelGGL(ebc::cadrl_grad_kernel, dim3((unsigned)now), dim3(64 * EBC_CADRL_GRAD_WAVES), lds, st, n->P, a);
      HIP_TRY(hipGetLastError());
    }
    const int first = done == 0, last = done + now >= chunks;
    hipLaunchKernelGGL(ebc::cadrl_grad_reduce, dim3(reduce_blocks), dim3(256), 0, st, partial, loss_part, count_part, now, PF, first, last, acc64,
                       args->grad, args->loss_sum, reinterpret_cast<long long *>(args->count));
    HIP_TRY(hipGetLastError());
    done += now;
  } while (done < chunks);
  return EBC_OK;
}
