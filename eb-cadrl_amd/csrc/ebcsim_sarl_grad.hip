// ebcsim_sarl_grad.hip — training the SARL value network: the network object ebc_sarl_net_* (the packed image of
// ebc_sarl_grad_rule.h in device memory, with the scratch of the chunk partials) and ebc_sarl_grad (the fused forward +
// backward kernel and the reduction of its partials, ebc_sarl_grad.h).  Its own translation unit: the deciding blocks keep
// their code.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_grad_host.h"
#include "ebc_sarl_grad.h"
#include "ebc_sarl_net.h"

namespace {

using ebc_host::fail;
using ebc_host::SarlNet;  // ebc_sarl_net.h: also what ebc_sarl_net_create_layers makes (ebcsim_sarl_grad_layers.hip)

constexpr int kMaxChunksPerLaunch = EBC_SARL_GRAD_MAX_CHUNKS;

}  // namespace

// ebc_sarl_net_create (om_width 0) and ebc_sarl_net_create_om; `what` names the entry in a refusal
static int net_create(const EbcSarlNetWeights *weights, int om_width, int device_id, void **net_out, const char *what) {
  const std::string who = std::string(what) + ": ";
  if (!weights || weights->struct_size != sizeof(EbcSarlNetWeights)) return fail(EBC_ERR_INVALID, "EbcSarlNetWeights.struct_size");
  if (!net_out) return fail(EBC_ERR_INVALID, who + "null net_out");
  const EbcSarlNetWeights &w = *weights;
  if (w.n_mlp1 != 2 || w.n_mlp2 != 2 || w.n_attention != 3 || w.n_mlp3 != 4)
    return fail(EBC_ERR_UNSUPPORTED, who + "mlp1 / mlp2 / attention / mlp3 have " + std::to_string(w.n_mlp1) + " / " +
                                         std::to_string(w.n_mlp2) + " / " + std::to_string(w.n_attention) + " / " + std::to_string(w.n_mlp3) +
                                         " Linear layers, the gradient takes exactly 2 / 2 / 3 / 4");
  int widths[EBC_SARL_GRAD_LAYERS + 1];
  widths[0] = w.input_dim;
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l) widths[l + 1] = w.widths[l];
  const int bad = ebc_sarl::grad_dims_refused_wide(widths, w.self_state_dim, om_width);
  if (bad == 1)
    return fail(EBC_ERR_UNSUPPORTED, who + "rows of " + std::to_string(widths[0]) + " floats, the gradient takes 1 .. " +
                                         std::to_string(EBC_SARL_GRAD_MAX_IN));
  if (bad == 14)
    return fail(EBC_ERR_UNSUPPORTED, who + "om_width " + std::to_string(om_width) + " outside 0 .. " + std::to_string(EBC_SARL_GRAD_MAX_OM));
  if (bad == 15)
    return fail(EBC_ERR_UNSUPPORTED, who + "T + om_width = " + std::to_string(widths[0] + om_width) + " columns, the gradient takes up to " +
                                         std::to_string(EBC_SARL_GRAD_MAX_WIDE));
  if (bad == 13)
    return fail(EBC_ERR_UNSUPPORTED, who + "self_state_dim " + std::to_string(w.self_state_dim) + " outside 0 .. the row width");
  if (bad == ebc_sarl::L_ATC + 2 || bad == ebc_sarl::L_M3D + 2)
    return fail(EBC_ERR_UNSUPPORTED, who + "the last layer of " + std::string(bad == ebc_sarl::L_ATC + 2 ? "attention" : "mlp3") + " has " +
                                         std::to_string(widths[bad - 1]) + " outputs, the gradient takes exactly 1");
  if (bad)
    return fail(EBC_ERR_UNSUPPORTED, who + "layer " + std::to_string(bad - 1) + " (counted through mlp1, mlp2, attention, mlp3) has " +
                                         std::to_string(widths[bad - 1]) + " units, the gradient takes 1 .. " + std::to_string(EBC_SARL_GRAD_MAX_WIDTH));
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l)
    if (!w.weight[l] || !w.bias[l]) return fail(EBC_ERR_INVALID, who + "null weight or bias of layer " + std::to_string(l + 1));
  HIP_TRY(hipSetDevice(device_id));
  SarlNet *n = new SarlNet;
  n->device = device_id;
  widths[0] += om_width;  // the rows the gradient reads: the rotated columns, then the map
  n->D = ebc_sarl::grad_dims(widths, w.self_state_dim, w.with_global_state);
  n->fill(EBC_SARL_GRAD_CHUNK, [n](int sp) { return ebc::sarl_grad_max_rows(n->D, sp); });
  std::vector<float> image(n->D.floats);
  ebc_sarl::grad_pack(n->D, w.weight, w.bias, image.data());
  return ebc_host::grad_net_upload(n, image, what, net_out);
}

extern "C" int ebc_sarl_net_create(const EbcSarlNetWeights *weights, int device_id, void **net_out) {
  return net_create(weights, 0, device_id, net_out, "ebc_sarl_net_create");
}

extern "C" int ebc_sarl_net_create_om(const EbcSarlNetWeights *weights, int om_width, int device_id, void **net_out) {
  return net_create(weights, om_width, device_id, net_out, "ebc_sarl_net_create_om");
}

extern "C" int ebc_sarl_net_destroy(void *net) { return ebc_host::grad_net_destroy(static_cast<SarlNet *>(net)); }

extern "C" int ebc_sarl_net_packed_floats(void *net, int64_t *floats_out) {
  return ebc_host::grad_net_packed_floats(static_cast<SarlNet *>(net), floats_out, "ebc_sarl_net_packed_floats");
}

extern "C" int ebc_sarl_net_grad_max_rows(void *net, int *rows_out) {
  if (!net || !rows_out) return fail(EBC_ERR_INVALID, "ebc_sarl_net_grad_max_rows: null argument");
  *rows_out = static_cast<SarlNet *>(net)->max_rows;
  return EBC_OK;
}

extern "C" int ebc_sarl_net_grad_max_rows_at(void *net, int states_per_pass, int *rows_out) {
  if (net && static_cast<SarlNet *>(net)->layers_grad && ebc_host::GradPasses::pass_index(states_per_pass) >= 0)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_net_grad_max_rows_at: states_per_pass " + std::to_string(states_per_pass) +
                                         ": the layer form has no passes");
  return ebc_host::grad_max_rows_at(static_cast<SarlNet *>(net), states_per_pass, rows_out, "ebc_sarl_net_grad_max_rows_at");
}

extern "C" int ebc_sarl_net_get_packed(void *net, void *stream, float *dst_dev) {
  return ebc_host::grad_net_copy_packed(static_cast<SarlNet *>(net), stream, dst_dev, nullptr, "ebc_sarl_net_get_packed");
}

extern "C" int ebc_sarl_net_set_packed(void *net, void *stream, const float *src_dev) {
  return ebc_host::grad_net_copy_packed(static_cast<SarlNet *>(net), stream, nullptr, src_dev, "ebc_sarl_net_set_packed");
}

extern "C" int ebc_sarl_grad(void *net, void *stream, const EbcSarlGradArgs *args) {
  if (!net) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcSarlGradArgs)) return fail(EBC_ERR_INVALID, "EbcSarlGradArgs.struct_size");
  if (!args->grad || !args->loss_sum || !args->count || args->B < 0) return fail(EBC_ERR_INVALID, "ebc_sarl_grad: grad, loss_sum, count, B");
  if (args->B > 0 && (!args->rows || !args->target)) return fail(EBC_ERR_INVALID, "ebc_sarl_grad: rows, target");
  if (static_cast<SarlNet *>(net)->layers_grad) return static_cast<SarlNet *>(net)->layers_grad(static_cast<SarlNet *>(net), stream, args);
  const int sp = args->states_per_pass;  // 0: the whole chunk at once, today's kernel
  if (int rc = ebc_host::GradPasses::check(sp, "ebc_sarl_grad")) return rc;
  SarlNet *n = static_cast<SarlNet *>(net);
  const ebc_sarl::GradDims &D = n->D;
  if (args->T != D.T)
    return fail(EBC_ERR_INVALID, "ebc_sarl_grad: rows are " + std::to_string(args->T) + " wide, the network takes " + std::to_string(D.T));
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: R < 1 row slots per state (" + std::to_string(args->R) + ")");
  if (int rc = n->refuse_rows(args->R, sp, EBC_SARL_GRAD_LDS_BYTES / 1024, "ebc_sarl_grad")) return rc;
  if (ebc_host::capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  // <= 160 KB: R <= max_rows, or max_rows_at of this pass size
  const size_t lds = ebc::sarl_grad_lds_floats(D, args->R, sp ? sp : EBC_SARL_GRAD_CHUNK) * sizeof(float);
  const auto kernel = sp ? ebc::sarl_grad_kernel<true> : ebc::sarl_grad_kernel<false>;
  static size_t raised_dev[2][64] = {{0}, {0}};  // the attribute is per kernel and device
  HIP_TRY(ebc_host::raise_dynamic_lds(kernel, n->device, lds, raised_dev[sp ? 1 : 0]));
  ebc::SarlGradLaunch a;
  a.rows = args->rows;
  a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
  a.target = args->target;
  a.mask = args->sample_mask;
  a.value = args->value;
  a.attention = args->attention;
  a.grad_scale = args->grad_scale;
  a.B = args->B;
  a.R = args->R;
  a.SP = sp;
  a.D = D;
  const auto scratch = [n](size_t bytes, void **out) { return ebc_host::grad_net_scratch(n, bytes, out); };
  const auto launch = [&](int chunk0, int now, float *partial, double *loss_part, long long *count_part) {
    a.partial = partial, a.loss_part = loss_part, a.count_part = count_part, a.chunk0 = chunk0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)now), dim3(64 * EBC_SARL_GRAD_WAVES), lds, st, n->P, a);
  };
  return ebc_host::grad_launch<true>(st, D.floats, args->B, EBC_SARL_GRAD_CHUNK, kMaxChunksPerLaunch, scratch, args->grad, args->loss_sum,
                                     args->count, launch);
}
