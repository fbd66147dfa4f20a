// ebcsim_lstm_grad.hip — training the LSTM-RL value networks: the network object ebc_lstm_net_* (the packed image of
// ebc_lstm_grad_rule.h in device memory, with the scratch of the chunk partials) and ebc_lstm_grad (the fused forward +
// backward-through-time kernel and the reduction of its partials, ebc_lstm_grad.h).  Its own translation unit: the scan
// that decides (ebcsim_lstm.hip) keeps its code.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_host.h"
#include "ebc_lstm_grad.h"

namespace {

using ebc_host::fail;

constexpr int kMaxChunksPerLaunch = EBC_LSTM_GRAD_MAX_CHUNKS;

struct LstmNet {
  int device = 0;
  ebc_lstmg::GradDims D;
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
  n->max_rows = ebc::lstm_grad_max_rows(n->D);
  for (int sp = 4, i = 0; sp >= 1; sp /= 2, ++i) n->max_rows_at[i] = ebc::lstm_grad_max_rows(n->D, sp);
  std::vector<float> image(n->D.floats);
  ebc_lstmg::grad_pack(n->D, w.weight, w.bias, w.w_ih, w.w_hh, w.b_ih, w.b_hh, image.data());
  hipError_t err = hipMalloc(&n->P, image.size() * sizeof(float));
  if (err == hipSuccess) err = hipMemcpy(n->P, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (n->P) (void)hipFree(n->P);
    delete n;
    return fail(EBC_ERR_DEVICE, std::string("ebc_lstm_net_create: ") + hipGetErrorString(err));
  }
  *net_out = n;
  return EBC_OK;
}

extern "C" int ebc_lstm_net_destroy(void *net) {
  if (!net) return EBC_OK;
  LstmNet *n = static_cast<LstmNet *>(net);
  (void)hipSetDevice(n->device);
  if (n->scratch) (void)hipFree(n->scratch);
  if (n->P) (void)hipFree(n->P);
  delete n;
  return EBC_OK;
}

extern "C" int ebc_lstm_net_packed_floats(void *net, int64_t *floats_out) {
  if (!net || !floats_out) return fail(EBC_ERR_INVALID, "ebc_lstm_net_packed_floats: null argument");
  *floats_out = (int64_t)static_cast<LstmNet *>(net)->D.floats;
  return EBC_OK;
}

extern "C" int ebc_lstm_net_grad_max_rows(void *net, int *rows_out) {
  if (!net || !rows_out) return fail(EBC_ERR_INVALID, "ebc_lstm_net_grad_max_rows: null argument");
  *rows_out = static_cast<LstmNet *>(net)->max_rows;
  return EBC_OK;
}

extern "C" int ebc_lstm_net_grad_max_rows_at(void *net, int states_per_pass, int *rows_out) {
  if (!net || !rows_out) return fail(EBC_ERR_INVALID, "ebc_lstm_net_grad_max_rows_at: null argument");
  const int i = pass_index(states_per_pass);
  if (states_per_pass != 0 && i < 0)
    return fail(EBC_ERR_INVALID, "ebc_lstm_net_grad_max_rows_at: states_per_pass " + std::to_string(states_per_pass) + " is none of 0, 4, 2, 1");
  const LstmNet *n = static_cast<LstmNet *>(net);
  *rows_out = states_per_pass == 0 ? n->max_rows : n->max_rows_at[i];
  return EBC_OK;
}

extern "C" int ebc_lstm_net_get_packed(void *net, void *stream, float *dst_dev) {
  if (!net || !dst_dev) return fail(EBC_ERR_INVALID, "ebc_lstm_net_get_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_get_packed: the stream is being captured into a HIP graph");
  LstmNet *n = static_cast<LstmNet *>(net);
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipMemcpyAsync(dst_dev, n->P, (size_t)n->D.floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_lstm_net_set_packed(void *net, void *stream, const float *src_dev) {
  if (!net || !src_dev) return fail(EBC_ERR_INVALID, "ebc_lstm_net_set_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_net_set_packed: the stream is being captured into a HIP graph");
  LstmNet *n = static_cast<LstmNet *>(net);
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipMemcpyAsync(n->P, src_dev, (size_t)n->D.floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_lstm_grad(void *net, void *stream, const EbcLstmGradArgs *args) {
  if (!net) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcLstmGradArgs)) return fail(EBC_ERR_INVALID, "EbcLstmGradArgs.struct_size");
  if (!args->grad || !args->loss_sum || !args->count || args->B < 0) return fail(EBC_ERR_INVALID, "ebc_lstm_grad: grad, loss_sum, count, B");
  if (args->B > 0 && (!args->rows || !args->target)) return fail(EBC_ERR_INVALID, "ebc_lstm_grad: rows, target");
  const int sp = args->states_per_pass, pi = pass_index(sp);  // 0: the whole chunk at once, today's kernel
  if (sp != 0 && pi < 0) return fail(EBC_ERR_INVALID, "ebc_lstm_grad: states_per_pass " + std::to_string(sp) + " is none of 0, 4, 2, 1");
  LstmNet *n = static_cast<LstmNet *>(net);
  const ebc_lstmg::GradDims &D = n->D;
  if (args->T != D.T)
    return fail(EBC_ERR_INVALID, "ebc_lstm_grad: rows are " + std::to_string(args->T) + " wide, the network takes " + std::to_string(D.T));
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_grad: R < 1 row slots per state (" + std::to_string(args->R) + ")");
  if (sp == 0 && args->R > n->max_rows)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_grad: R = " + std::to_string(args->R) + " row slots per state, a chunk of this network fits a workgroup's " +
                                         std::to_string(EBC_LSTM_GRAD_LDS_BYTES / 1024) + " KB of LDS up to R = " + std::to_string(n->max_rows));
  if (sp != 0 && args->R > n->max_rows_at[pi])
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_grad: R = " + std::to_string(args->R) + " row slots per state with S = " + std::to_string(sp) +
                                         " states per pass, that many states of this network fit a workgroup's " +
                                         std::to_string(EBC_LSTM_GRAD_LDS_BYTES / 1024) + " KB of LDS up to R = " + std::to_string(n->max_rows_at[pi]));
  if (capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_lstm_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t PF = D.floats;
  const int B = args->B;
  const long long chunks = ((long long)B + EBC_LSTM_GRAD_CHUNK - 1) / EBC_LSTM_GRAD_CHUNK;
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
  const size_t lds = ebc::lstm_grad_lds_floats(D, args->R, sp ? sp : EBC_LSTM_GRAD_CHUNK) * sizeof(float);
  const auto kernel = sp ? ebc::lstm_grad_kernel<true> : ebc::lstm_grad_kernel<false>;
  static size_t raised_dev[2][64] = {{0}, {0}};  // the attribute is per kernel and device
  HIP_TRY(ebc_host::raise_dynamic_lds(kernel, n->device, lds, raised_dev[sp ? 1 : 0]));
  const unsigned reduce_blocks = (unsigned)((PF + 255) / 256);
  long long done = 0;
  do {
    const int now = chunks - done < per ? (int)(chunks - done) : per;
    if (now > 0) {
      ebc::LstmGradLaunch a;
      a.rows = args->rows;
      a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
      a.target = args->target;
      a.mask = args->sample_mask;
      a.value = args->value;
      a.joint = args->joint;
      a.partial = partial;
      a.loss_part = loss_part;
      a.count_part = count_part;
      a.grad_scale = args->grad_scale;
      a.B = B;
      a.R = args->R;
      a.chunk0 = (int)done;
      a.SP = sp;
      a.D = D;
      hipLaunchKernelGGL(kernel, dim3((unsigned)now), dim3(64 * EBC_LSTM_GRAD_WAVES), lds, st, n->P, a);
      HIP_TRY(hipGetLastError());
    }
    const int first = done == 0, last = done + now >= chunks;
    hipLaunchKernelGGL(ebc::lstm_grad_reduce, dim3(reduce_blocks), dim3(256), 0, st, partial, loss_part, count_part, now, PF, first, last, acc64,
                       args->grad, args->loss_sum, reinterpret_cast<long long *>(args->count));
    HIP_TRY(hipGetLastError());
    done += now;
  } while (done < chunks);
  return EBC_OK;
}
