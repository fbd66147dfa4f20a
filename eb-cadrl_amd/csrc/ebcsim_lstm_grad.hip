// ebcsim_lstm_grad.hip — training the LSTM-RL value networks: the network object ebc_lstm_net_* (the packed image of
// ebc_lstm_grad_rule.h in device memory, with the scratch of the chunk partials) and ebc_lstm_grad (the fused forward +
// backward-through-time kernel and the reduction of its partials, ebc_lstm_grad.h).  Its own translation unit: the scan
// that decides (ebcsim_lstm.hip) keeps its code.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_grad_host.h"
#include "ebc_lstm_grad.h"

namespace {

using ebc_host::fail;

constexpr int kMaxChunksPerLaunch = EBC_LSTM_GRAD_MAX_CHUNKS;

struct LstmNet : ebc_host::GradNet, ebc_host::GradPasses {
  ebc_lstmg::GradDims D;
};

}  // namespace

extern "C" int ebc_lstm_net_create(const EbcLstmNetWeights *weights, int device_id, void **net_out) {
  if (!weights || weights->struct_size != sizeof(EbcLstmNetWeights)) return fail(EBC_ERR_INVALID, "EbcLstmNetWeights.struct_size");
  if (!net_out) return fail(EBC_ERR_INVALID, "ebc_lstm_net_create: null net_out");
  const EbcLstmNetWeights &w = *weights;
  if ((w.n_mlp1 != 0 && w.n_mlp1 != 4) || w.n_mlp != 4)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: mlp1 / mlp have " + std::to_string(w.n_mlp1) + " / " + std::to_string(w.n_mlp) +
                                         " Linear layers, the gradient takes 0 or 4 / 4");
  const int two = w.n_mlp1 == 4;
  int widths[10];
  widths[0] = w.input_dim;
  for (int l = 0; l < 4; ++l) widths[1 + l] = two ? w.widths[l] : 0;
  widths[5] = w.hidden_dim;
  for (int l = 0; l < 4; ++l) widths[6 + l] = w.widths[4 + l];
  const int bad = ebc_lstmg::grad_dims_refused(widths, w.self_state_dim, two);
  if (bad == 1)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: rows of " + std::to_string(widths[0]) + " floats, the gradient takes 1 .. " +
                                         std::to_string(EBC_LSTM_GRAD_MAX_IN));
  if (bad == 6)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: the LSTM's input is " + std::to_string(two ? widths[4] : widths[0]) +
                                         " wide, the gradient takes 1 .. " + std::to_string(EBC_LSTM_MAX_DIM));
  if (bad == 7)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: lstm_hidden_dim " + std::to_string(widths[5]) + ", the gradient takes 1 .. " +
                                         std::to_string(EBC_LSTM_MAX_DIM));
  if (bad == 12)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: self_state_dim " + std::to_string(w.self_state_dim) + " outside 0 .. the row width");
  if (bad == 11 && widths[9] >= 1 && widths[9] <= EBC_LSTM_GRAD_MAX_WIDTH)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: the last layer of mlp has " + std::to_string(widths[9]) + " outputs, the gradient takes exactly 1");
  if (bad)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_create: layer " + std::to_string(bad < 6 ? bad - 1 : bad - 7) + " of " + (bad < 6 ? "mlp1" : "mlp") + " has " +
                                         std::to_string(widths[bad < 6 ? bad - 1 : bad - 2]) + " units, the gradient takes 1 .. " +
                                         std::to_string(EBC_LSTM_GRAD_MAX_WIDTH));
  const int I = two ? widths[4] : widths[0];
  if (w.lstm_input_dim != I)
    return fail(EBC_ERR_INVALID, "ebc_lstm_net_create: the LSTM takes " + std::to_string(w.lstm_input_dim) + " inputs, " +
                                     (two ? "mlp1 gives " : "the rows are ") + std::to_string(I));
  for (int l = two ? 0 : 4; l < EBC_LSTM_GRAD_LAYERS; ++l)
    if (!w.weight[l] || !w.bias[l]) return fail(EBC_ERR_INVALID, "ebc_lstm_net_create: null weight or bias of Linear layer " + std::to_string(l));
  if (!w.w_ih || !w.w_hh || !w.b_ih || !w.b_hh) return fail(EBC_ERR_INVALID, "ebc_lstm_net_create: null w_ih, w_hh, b_ih or b_hh");
  HIP_TRY(hipSetDevice(device_id));
  LstmNet *n = new LstmNet;
  n->device = device_id;
  n->D = ebc_lstmg::grad_dims(widths, w.self_state_dim, two);
  n->fill(EBC_LSTM_GRAD_CHUNK, [n](int sp) { return ebc::lstm_grad_max_rows(n->D, sp); });
  std::vector<float> image(n->D.floats);
  ebc_lstmg::grad_pack(n->D, w.weight, w.bias, w.w_ih, w.w_hh, w.b_ih, w.b_hh, image.data());
  return ebc_host::grad_net_upload(n, image, "ebc_lstm_net_create", net_out);
}

extern "C" int ebc_lstm_net_destroy(void *net) { return ebc_host::grad_net_destroy(static_cast<LstmNet *>(net)); }

extern "C" int ebc_lstm_net_packed_floats(void *net, int64_t *floats_out) {
  return ebc_host::grad_net_packed_floats(static_cast<LstmNet *>(net), floats_out, "ebc_lstm_net_packed_floats");
}

extern "C" int ebc_lstm_net_grad_max_rows(void *net, int *rows_out) {
  if (!net || !rows_out) return fail(EBC_ERR_INVALID, "ebc_lstm_net_grad_max_rows: null argument");
  *rows_out = static_cast<LstmNet *>(net)->max_rows;
  return EBC_OK;
}

extern "C" int ebc_lstm_net_grad_max_rows_at(void *net, int states_per_pass, int *rows_out) {
  return ebc_host::grad_max_rows_at(static_cast<LstmNet *>(net), states_per_pass, rows_out, "ebc_lstm_net_grad_max_rows_at");
}

extern "C" int ebc_lstm_net_get_packed(void *net, void *stream, float *dst_dev) {
  return ebc_host::grad_net_copy_packed(static_cast<LstmNet *>(net), stream, dst_dev, nullptr, "ebc_lstm_net_get_packed");
}

extern "C" int ebc_lstm_net_set_packed(void *net, void *stream, const float *src_dev) {
  return ebc_host::grad_net_copy_packed(static_cast<LstmNet *>(net), stream, nullptr, src_dev, "ebc_lstm_net_set_packed");
}

extern "C" int ebc_lstm_grad(void *net, void *stream, const EbcLstmGradArgs *args) {
  if (!net) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcLstmGradArgs)) return fail(EBC_ERR_INVALID, "EbcLstmGradArgs.struct_size");
  if (!args->grad || !args->loss_sum || !args->count || args->B < 0) return fail(EBC_ERR_INVALID, "ebc_lstm_grad: grad, loss_sum, count, B");
  if (args->B > 0 && (!args->rows || !args->target)) return fail(EBC_ERR_INVALID, "ebc_lstm_grad: rows, target");
  const int sp = args->states_per_pass;  // 0: the whole chunk at once, today's kernel
  if (int rc = ebc_host::GradPasses::check(sp, "ebc_lstm_grad")) return rc;
  LstmNet *n = static_cast<LstmNet *>(net);
  const ebc_lstmg::GradDims &D = n->D;
  if (args->T != D.T)
    return fail(EBC_ERR_INVALID, "ebc_lstm_grad: rows are " + std::to_string(args->T) + " wide, the network takes " + std::to_string(D.T));
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_grad: R < 1 row slots per state (" + std::to_string(args->R) + ")");
  if (int rc = n->refuse_rows(args->R, sp, EBC_LSTM_GRAD_LDS_BYTES / 1024, "ebc_lstm_grad")) return rc;
  if (ebc_host::capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  // <= 160 KB: R <= max_rows, or max_rows_at of this pass size
  const size_t lds = ebc::lstm_grad_lds_floats(D, args->R, sp ? sp : EBC_LSTM_GRAD_CHUNK) * sizeof(float);
  const auto kernel = sp ? ebc::lstm_grad_kernel<true> : ebc::lstm_grad_kernel<false>;
  static size_t raised_dev[2][64] = {{0}, {0}};  // the attribute is per kernel and device
  HIP_TRY(ebc_host::raise_dynamic_lds(kernel, n->device, lds, raised_dev[sp ? 1 : 0]));
  ebc::LstmGradLaunch a;
  a.rows = args->rows;
  a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
  a.target = args->target;
  a.mask = args->sample_mask;
  a.value = args->value;
  a.joint = args->joint;
  a.grad_scale = args->grad_scale;
  a.B = args->B;
  a.R = args->R;
  a.SP = sp;
  a.D = D;
  const auto scratch = [n](size_t bytes, void **out) { return ebc_host::grad_net_scratch(n, bytes, out); };
  const auto launch = [&](int chunk0, int now, float *partial, double *loss_part, long long *count_part) {
    a.partial = partial, a.loss_part = loss_part, a.count_part = count_part, a.chunk0 = chunk0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)now), dim3(64 * EBC_LSTM_GRAD_WAVES), lds, st, n->P, a);
  };
  return ebc_host::grad_launch<true>(st, D.floats, args->B, EBC_LSTM_GRAD_CHUNK, kMaxChunksPerLaunch, scratch, args->grad, args->loss_sum,
                                     args->count, launch);
}
