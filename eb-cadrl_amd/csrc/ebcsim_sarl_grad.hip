// ebcsim_sarl_grad.hip — training the SARL value network: the network object ebc_sarl_net_* (the packed image of
// ebc_sarl_grad_rule.h in device memory, with the scratch of the chunk partials) and ebc_sarl_grad (the fused forward +
// backward kernel and the reduction of its partials, ebc_sarl_grad.h).  Its own translation unit: the deciding blocks keep
// their code.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_host.h"
#include "ebc_sarl_grad.h"

namespace {

using ebc_host::fail;

constexpr int kMaxChunksPerLaunch = EBC_SARL_GRAD_MAX_CHUNKS;

struct SarlNet {
  int device = 0;
  ebc_sarl::GradDims D;
  int max_rows = 0;          // the largest R whose chunk fits a workgroup's LDS
  int max_rows_at[3] = {0, 0, 0};  // the same with 4, 2, 1 states per pass
  float *P = nullptr;        // the packed image
  void *scratch = nullptr;   // float64 sums | chunk losses | chunk counts | chunk partials
  size_t scratch_bytes = 0;
};

// states_per_pass 4, 2, 1 -> 0, 1, 2; anything else -1
int pass_index(int states_per_pass) {
  return states_per_pass == 4 ? 0 : states_per_pass == 2 ? 1 : states_per_pass == 1 ? 2 : -1;
}

bool capturing(void *stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

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
  n->max_rows = ebc::sarl_grad_max_rows(n->D);
  for (int sp = 4, i = 0; sp >= 1; sp /= 2, ++i) n->max_rows_at[i] = ebc::sarl_grad_max_rows(n->D, sp);
  std::vector<float> image(n->D.floats);
  ebc_sarl::grad_pack(n->D, w.weight, w.bias, image.data());
  hipError_t err = hipMalloc(&n->P, image.size() * sizeof(float));
  if (err == hipSuccess) err = hipMemcpy(n->P, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (n->P) (void)hipFree(n->P);
    delete n;
    return fail(EBC_ERR_DEVICE, who + hipGetErrorString(err));
  }
  *net_out = n;
  return EBC_OK;
}

extern "C" int ebc_sarl_net_create(const EbcSarlNetWeights *weights, int device_id, void **net_out) {
  return net_create(weights, 0, device_id, net_out, "ebc_sarl_net_create");
}

extern "C" int ebc_sarl_net_create_om(const EbcSarlNetWeights *weights, int om_width, int device_id, void **net_out) {
  return net_create(weights, om_width, device_id, net_out, "ebc_sarl_net_create_om");
}

extern "C" int ebc_sarl_net_destroy(void *net) {
  if (!net) return EBC_OK;
  SarlNet *n = static_cast<SarlNet *>(net);
  (void)hipSetDevice(n->device);
  if (n->scratch) (void)hipFree(n->scratch);
  if (n->P) (void)hipFree(n->P);
  delete n;
  return EBC_OK;
}

extern "C" int ebc_sarl_net_packed_floats(void *net, int64_t *floats_out) {
  if (!net || !floats_out) return fail(EBC_ERR_INVALID, "ebc_sarl_net_packed_floats: null argument");
  *floats_out = (int64_t)static_cast<SarlNet *>(net)->D.floats;
  return EBC_OK;
}

extern "C" int ebc_sarl_net_grad_max_rows(void *net, int *rows_out) {
  if (!net || !rows_out) return fail(EBC_ERR_INVALID, "ebc_sarl_net_grad_max_rows: null argument");
  *rows_out = static_cast<SarlNet *>(net)->max_rows;
  return EBC_OK;
}

extern "C" int ebc_sarl_net_grad_max_rows_at(void *net, int states_per_pass, int *rows_out) {
  if (!net || !rows_out) return fail(EBC_ERR_INVALID, "ebc_sarl_net_grad_max_rows_at: null argument");
  const int i = pass_index(states_per_pass);
  if (states_per_pass != 0 && i < 0)
    return fail(EBC_ERR_INVALID, "ebc_sarl_net_grad_max_rows_at: states_per_pass " + std::to_string(states_per_pass) + " is none of 0, 4, 2, 1");
  const SarlNet *n = static_cast<SarlNet *>(net);
  *rows_out = states_per_pass == 0 ? n->max_rows : n->max_rows_at[i];
  return EBC_OK;
}

extern "C" int ebc_sarl_net_get_packed(void *net, void *stream, float *dst_dev) {
  if (!net || !dst_dev) return fail(EBC_ERR_INVALID, "ebc_sarl_net_get_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_net_get_packed: the stream is being captured into a HIP graph");
  SarlNet *n = static_cast<SarlNet *>(net);
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipMemcpyAsync(dst_dev, n->P, (size_t)n->D.floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_sarl_net_set_packed(void *net, void *stream, const float *src_dev) {
  if (!net || !src_dev) return fail(EBC_ERR_INVALID, "ebc_sarl_net_set_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_net_set_packed: the stream is being captured into a HIP graph");
  SarlNet *n = static_cast<SarlNet *>(net);
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipMemcpyAsync(n->P, src_dev, (size_t)n->D.floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_sarl_grad(void *net, void *stream, const EbcSarlGradArgs *args) {
  if (!net) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcSarlGradArgs)) return fail(EBC_ERR_INVALID, "EbcSarlGradArgs.struct_size");
  if (!args->grad || !args->loss_sum || !args->count || args->B < 0) return fail(EBC_ERR_INVALID, "ebc_sarl_grad: grad, loss_sum, count, B");
  if (args->B > 0 && (!args->rows || !args->target)) return fail(EBC_ERR_INVALID, "ebc_sarl_grad: rows, target");
  const int sp = args->states_per_pass, pi = pass_index(sp);  // 0: the whole chunk at once, today's kernel
  if (sp != 0 && pi < 0) return fail(EBC_ERR_INVALID, "ebc_sarl_grad: states_per_pass " + std::to_string(sp) + " is none of 0, 4, 2, 1");
  SarlNet *n = static_cast<SarlNet *>(net);
  const ebc_sarl::GradDims &D = n->D;
  if (args->T != D.T)
    return fail(EBC_ERR_INVALID, "ebc_sarl_grad: rows are " + std::to_string(args->T) + " wide, the network takes " + std::to_string(D.T));
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: R < 1 row slots per state (" + std::to_string(args->R) + ")");
  if (sp == 0 && args->R > n->max_rows)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: R = " + std::to_string(args->R) + " row slots per state, a chunk of this network fits a workgroup's " +
                                         std::to_string(EBC_SARL_GRAD_LDS_BYTES / 1024) + " KB of LDS up to R = " + std::to_string(n->max_rows));
  if (sp != 0 && args->R > n->max_rows_at[pi])
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: R = " + std::to_string(args->R) + " row slots per state with S = " + std::to_string(sp) +
                                         " states per pass, that many states of this network fit a workgroup's " +
                                         std::to_string(EBC_SARL_GRAD_LDS_BYTES / 1024) + " KB of LDS up to R = " + std::to_string(n->max_rows_at[pi]));
  if (capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t PF = D.floats;
  const int B = args->B;
  const long long chunks = ((long long)B + EBC_SARL_GRAD_CHUNK - 1) / EBC_SARL_GRAD_CHUNK;
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

  // <= 160 KB: R <= max_rows, or max_rows_at of this pass size
  const size_t lds = ebc::sarl_grad_lds_floats(D, args->R, sp ? sp : EBC_SARL_GRAD_CHUNK) * sizeof(float);
  const auto kernel = sp ? ebc::sarl_grad_kernel<true> : ebc::sarl_grad_kernel<false>;
  static size_t raised_dev[2][64] = {{0}, {0}};  // the attribute is per kernel and device
  HIP_TRY(ebc_host::raise_dynamic_lds(kernel, n->device, lds, raised_dev[sp ? 1 : 0]));
  const unsigned reduce_blocks = (unsigned)((PF + 255) / 256);
  long long done = 0;
  do {
    const int now = chunks - done < per ? (int)(chunks - done) : per;
    if (now > 0) {
      ebc::SarlGradLaunch a;
      a.rows = args->rows;
      a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
      a.target = args->target;
      a.mask = args->sample_mask;
      a.value = args->value;
      a.attention = args->attention;
      a.partial = partial;
      a.loss_part = loss_part;
      a.count_part = count_part;
      a.grad_scale = args->grad_scale;
      a.B = B;
      a.R = args->R;
      a.chunk0 = (int)done;
      a.SP = sp;
      a.D = D;
      hipLaunchKernelGGL(kernel, dim3((unsigned)now), dim3(64 * EBC_SARL_GRAD_WAVES), lds, st, n->P, a);
      HIP_TRY(hipGetLastError());
    }
    const int first = done == 0, last = done + now >= chunks;
    hipLaunchKernelGGL(ebc::sarl_grad_reduce, dim3(reduce_blocks), dim3(256), 0, st, partial, loss_part, count_part, now, PF, first, last, acc64,
                       args->grad, args->loss_sum, reinterpret_cast<long long *>(args->count));
    HIP_TRY(hipGetLastError());
    done += now;
  } while (done < chunks);
  return EBC_OK;
}
