// ebcsim_cadrl_grad.hip — training the CADRL value network: the network object ebc_cadrl_net_* (the packed image of
// ebc_cadrl_grad_rule.h in device memory, with the scratch of the chunk partials) and ebc_cadrl_grad (the fused forward +
// minimum + backward kernel and the reduction of its partials, ebc_cadrl_grad.h).  Its own translation unit: the decision's
// unit and the two-layer blocks keep their code.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_cadrl_grad.h"
#include "ebc_grad_host.h"

namespace {

using ebc_host::fail;

constexpr int kMaxChunksPerLaunch = 1024;  // 1024 chunks of partials (114 MB at the reference widths) before the float64 sums take over

struct CadrlNet : ebc_host::GradNet {
  ebc_cadrl::GradDims D;
};

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
  return ebc_host::grad_net_upload(n, image, "ebc_cadrl_net_create", net_out);
}

extern "C" int ebc_cadrl_net_destroy(void *net) { return ebc_host::grad_net_destroy(static_cast<CadrlNet *>(net)); }

extern "C" int ebc_cadrl_net_packed_floats(void *net, int64_t *floats_out) {
  return ebc_host::grad_net_packed_floats(static_cast<CadrlNet *>(net), floats_out, "ebc_cadrl_net_packed_floats");
}

extern "C" int ebc_cadrl_net_get_packed(void *net, void *stream, float *dst_dev) {
  return ebc_host::grad_net_copy_packed(static_cast<CadrlNet *>(net), stream, dst_dev, nullptr, "ebc_cadrl_net_get_packed");
}

extern "C" int ebc_cadrl_net_set_packed(void *net, void *stream, const float *src_dev) {
  return ebc_host::grad_net_copy_packed(static_cast<CadrlNet *>(net), stream, nullptr, src_dev, "ebc_cadrl_net_set_packed");
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
  if (ebc_host::capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t lds = ebc::cadrl_grad_lds_floats(D, args->R) * sizeof(float);  // <= 115 KB
  static size_t raised_dev[64] = {0};
  HIP_TRY(ebc_host::raise_dynamic_lds(ebc::cadrl_grad_kernel, n->device, lds, raised_dev));
  ebc::CadrlGradLaunch a;
  a.rows = args->rows;
  a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
  a.target = args->target;
  a.mask = args->sample_mask;
  a.value = args->value;
  a.min_row = args->min_row;
  a.grad_scale = args->grad_scale;
  a.B = args->B;
  a.R = args->R;
  a.D = D;
  const auto scratch = [n](size_t bytes, void **out) { return ebc_host::grad_net_scratch(n, bytes, out); };
  const auto launch = [&](int chunk0, int now, float *partial, double *loss_part, long long *count_part) {
    a.partial = partial, a.loss_part = loss_part, a.count_part = count_part, a.chunk0 = chunk0;
    hipLaunchKernelGGL(ebc::cadrl_grad_kernel, dim3((unsigned)now), dim3(64 * EBC_CADRL_GRAD_WAVES), lds, st, n->P, a);
  };
  return ebc_host::grad_launch<true>(st, D.floats, args->B, EBC_CADRL_GRAD_CHUNK, kMaxChunksPerLaunch, scratch, args->grad, args->loss_sum,
                                     args->count, launch);
}
