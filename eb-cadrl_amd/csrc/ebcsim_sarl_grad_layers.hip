// ebcsim_sarl_grad_layers.hip — the layer form of the SARL gradient: ebc_sarl_net_create_layers (a network object of
// ebcsim_sarl_grad.hip's kind, same packed image, hidden layers up to 640) and the body ebc_sarl_grad runs on such a network:
// the kernels of ebc_sarl_grad_layers.h, launched layer by layer over runs of whole chunks.  Its own translation unit.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_sarl_grad_layers.h"
#include "ebc_sarl_net.h"

namespace {

using ebc_host::fail;
using ebc_host::SarlNet;
using namespace ebc_sarl;

constexpr int kChunk = EBC_SARL_GRAD_CHUNK;

// the scratch of a run of Bp states: carved in order, every piece 256-byte aligned
struct Carve {
  size_t at = 0;
  char *base = nullptr;
  template <class T>
  T *take(size_t count) {
    T *p = reinterpret_cast<T *>(base + at);
    at += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

struct RunBuffers {
  double *acc64, *LOSS;
  int *N, *LIVE, *SLOT;
  float *A1, *H1, *B1, *FT, *C1, *C2, *SC, *WT, *D2, *D4, *G, *GQ, *J, *DJ, *M1, *M2, *M3, *OUT, *SEED;
  int s[EBC_SARL_GRAD_LAYERS], js, d4s;  // strides: layer l's output, the joint vector, attention layer 0's dx

  size_t lay(char *base, const GradDims &D, size_t Bp, size_t R) {
    Carve c;
    c.base = base;
    const size_t Q = Bp * R;
    for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l) s[l] = pad4(D.O[l]);
    js = pad4(D.K[L_M3A]), d4s = pad4(D.K[L_ATA]);
    acc64 = c.take<double>(D.floats + 2);
    LOSS = c.take<double>(Bp);
    N = c.take<int>(Bp), LIVE = c.take<int>(Bp), SLOT = c.take<int>(Q);
    A1 = c.take<float>(Q * s[L_M1A]), H1 = c.take<float>(Q * s[L_M1B]), B1 = c.take<float>(Q * s[L_M2A]), FT = c.take<float>(Q * s[L_M2B]);
    C1 = c.take<float>(Q * s[L_ATA]), C2 = c.take<float>(Q * s[L_ATB]), SC = c.take<float>(Q), WT = c.take<float>(Q);
    D2 = c.take<float>(Q * s[L_M1B]), D4 = c.take<float>(Q * d4s);
    G = c.take<float>(Bp * s[L_M1B]), GQ = c.take<float>(Q * s[L_M1B]), J = c.take<float>(Bp * js), DJ = c.take<float>(Bp * js);
    M1 = c.take<float>(Bp * s[L_M3A]), M2 = c.take<float>(Bp * s[L_M3B]), M3 = c.take<float>(Bp * s[L_M3C]);
    OUT = c.take<float>(Bp), SEED = c.take<float>(Bp);
    return c.at;
  }
};

unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// ebc_sarl_grad on a network of ebc_sarl_net_create_layers; net, args and args->struct_size are checked
int layers_grad(SarlNet *n, void *stream, const EbcSarlGradArgs *args) {
  const GradDims &D = n->D;
  const int sp = args->states_per_pass;
  if (sp == 4 || sp == 2 || sp == 1)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: states_per_pass " + std::to_string(sp) + ": the layer form has no passes");
  if (int rc = ebc_host::GradPasses::check(sp, "ebc_sarl_grad")) return rc;
  if (args->T != D.T)
    return fail(EBC_ERR_INVALID, "ebc_sarl_grad: rows are " + std::to_string(args->T) + " wide, the network takes " + std::to_string(D.T));
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: R < 1 row slots per state (" + std::to_string(args->R) + ")");
  if (args->R > EBC_SARL_GRAD_LAYERS_MAX_ROWS)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: R = " + std::to_string(args->R) + " row slots per state, the layer form takes up to R = " +
                                         std::to_string(EBC_SARL_GRAD_LAYERS_MAX_ROWS));
  if (ebc_host::capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sarl_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(n->device));
  const hipStream_t st = (hipStream_t)stream;
  const long long B = args->B;
  const int R = args->R, T = D.T;
  long long *count = reinterpret_cast<long long *>(args->count);
  if (B == 0) {
    hipLaunchKernelGGL(ebc::layers_empty, dim3(blocks_of(D.floats, 256)), dim3(256), 0, st, (size_t)D.floats, args->grad, args->loss_sum, count);
    HIP_TRY(hipGetLastError());
    return EBC_OK;
  }
  // runs of whole chunks, at most RUN_SLOTS row slots each (one chunk at the least)
  long long per = EBC_SARL_GRAD_LAYERS_RUN_SLOTS / R / kChunk * kChunk;
  if (per < kChunk) per = kChunk;
  if (per > B) per = B;
  RunBuffers m;
  void *mem = nullptr;
  if (int rc = ebc_host::grad_net_scratch(n, m.lay(nullptr, D, (size_t)per, (size_t)R), &mem)) return rc;
  m.lay(static_cast<char *>(mem), D, (size_t)per, (size_t)R);
  const float *P = n->P;
  const int H = D.O[L_M1B], F = D.O[L_M2B], S = D.S;

  for (long long b0 = 0; b0 < B; b0 += per) {
    const int Bp = (int)(B - b0 < per ? B - b0 : per);
    const long long Q = (long long)Bp * R;
    const int first = b0 == 0, last = b0 + per >= B;
    const float *rows = args->rows + (size_t)b0 * R * T;
    // Y = [relu] layer l of X (K2 further inputs from X2, one row per R of X's)
    const auto forward = [&](int l, bool relu, const float *X, int xs, const float *X2, int x2s, int K2, float *Y, int ys, long long rowsQ) {
      const dim3 grid(blocks_of(rowsQ, 128), blocks_of(D.O[l], 64));
      const auto k = relu ? ebc::layers_forward<true> : ebc::layers_forward<false>;
      hipLaunchKernelGGL(k, grid, dim3(256), 0, st, P + D.at[l], D.K[l] - K2, K2, D.O[l], D.Op[l], X, xs, X2, x2s, R, Y, ys, rowsQ);
    };
    // out = dx of layer l from delta (relu: through the ReLU of the activation in `out`, whose place it takes)
    const auto dx = [&](int l, bool relu, const float *delta, int ds, float *out, int os, long long rowsQ) {
      const dim3 grid(blocks_of(rowsQ, 128), blocks_of(D.K[l], 64));
      const auto k = relu ? ebc::layers_dx<true> : ebc::layers_dx<false>;
      hipLaunchKernelGGL(k, grid, dim3(256), 0, st, P + D.at[l], D.K[l], D.O[l], D.Op[l], delta, ds, out, os, out, os, rowsQ);
    };
    // layer l's dW and db from its input X (and X2) and its delta; per_row: over row slots, else over states
    const auto dw = [&](int l, const float *X, int xs, const float *X2, int x2s, int K2, const float *delta, int ds, bool per_row) {
      const dim3 grid(blocks_of(D.K[l] + 1, 32), blocks_of(D.Op[l], 32));
      hipLaunchKernelGGL(ebc::layers_dw, grid, dim3(64 * EBC_LAYERS_DW_WAVES), 0, st, X, xs, D.K[l] - K2, X2, x2s, K2, delta, ds, D.O[l], D.Op[l],
                         per_row ? m.SLOT : m.LIVE, per_row ? Q : (long long)Bp, per_row ? kChunk * R : kChunk, first, last, m.acc64 + D.at[l],
                         args->grad + D.at[l]);
    };
    const int *s = m.s;
    // ---- forward
    hipLaunchKernelGGL(ebc::layers_rows, dim3(blocks_of(Q, 256)), dim3(256), 0, st, reinterpret_cast<const long long *>(args->n_valid),
                       args->sample_mask, b0, Bp, R, m.N, m.LIVE, m.SLOT);
    forward(L_M1A, true, rows, T, nullptr, 0, 0, m.A1, s[L_M1A], Q);
    forward(L_M1B, true, m.A1, s[L_M1A], nullptr, 0, 0, m.H1, s[L_M1B], Q);
    forward(L_M2A, true, m.H1, s[L_M1B], nullptr, 0, 0, m.B1, s[L_M2A], Q);
    forward(L_M2B, false, m.B1, s[L_M2A], nullptr, 0, 0, m.FT, s[L_M2B], Q);
    if (D.global)
      hipLaunchKernelGGL(ebc::layers_mean, dim3(blocks_of((long long)Bp * H, 256)), dim3(256), 0, st, m.H1, s[L_M1B], H, R, m.N, Bp, m.G,
                         m.GQ, s[L_M1B]);
    forward(L_ATA, true, m.H1, s[L_M1B], m.G, s[L_M1B], D.global ? H : 0, m.C1, s[L_ATA], Q);
    forward(L_ATB, true, m.C1, s[L_ATA], nullptr, 0, 0, m.C2, s[L_ATB], Q);
    forward(L_ATC, false, m.C2, s[L_ATB], nullptr, 0, 0, m.SC, 1, Q);
    hipLaunchKernelGGL(ebc::layers_softmax, dim3((unsigned)Bp), dim3(128), 0, st, m.SC, m.FT, s[L_M2B], F, rows, T, S, R, m.N, m.WT,
                       args->attention ? args->attention + (size_t)b0 * R : nullptr, m.J, m.js);
    forward(L_M3A, true, m.J, m.js, nullptr, 0, 0, m.M1, s[L_M3A], Bp);
    forward(L_M3B, true, m.M1, s[L_M3A], nullptr, 0, 0, m.M2, s[L_M3B], Bp);
    forward(L_M3C, true, m.M2, s[L_M3B], nullptr, 0, 0, m.M3, s[L_M3C], Bp);
    forward(L_M3D, false, m.M3, s[L_M3C], nullptr, 0, 0, m.OUT, 1, Bp);
    hipLaunchKernelGGL(ebc::layers_seed, dim3(blocks_of(Bp, 256)), dim3(256), 0, st, m.OUT, m.N, m.LIVE, args->target, b0, Bp, args->grad_scale,
                       args->value, m.LOSS, m.SEED);
    hipLaunchKernelGGL(ebc::layers_loss, dim3(1), dim3(64), 0, st, m.LOSS, m.LIVE, Bp, kChunk, first, last, m.acc64 + D.floats, args->loss_sum,
                       count);
    HIP_TRY(hipGetLastError());
    // ---- backward, in the rule's order: a layer's dW reads its input before that input's delta takes its place
    dw(L_M3D, m.M3, s[L_M3C], nullptr, 0, 0, m.SEED, 1, false);
    dx(L_M3D, true, m.SEED, 1, m.M3, s[L_M3C], Bp);
    dw(L_M3C, m.M2, s[L_M3B], nullptr, 0, 0, m.M3, s[L_M3C], false);
    dx(L_M3C, true, m.M3, s[L_M3C], m.M2, s[L_M3B], Bp);
    dw(L_M3B, m.M1, s[L_M3A], nullptr, 0, 0, m.M2, s[L_M3B], false);
    dx(L_M3B, true, m.M2, s[L_M3B], m.M1, s[L_M3A], Bp);
    dw(L_M3A, m.J, m.js, nullptr, 0, 0, m.M1, s[L_M3A], false);
    dx(L_M3A, false, m.M1, s[L_M3A], m.DJ, m.js, Bp);
    hipLaunchKernelGGL(ebc::layers_softmax_back, dim3((unsigned)Bp), dim3(128), 0, st, m.DJ, m.J, m.js, S, F, R, m.N, m.WT, m.SC, m.FT,
                       s[L_M2B]);
    dw(L_M2B, m.B1, s[L_M2A], nullptr, 0, 0, m.FT, s[L_M2B], true);
    dx(L_M2B, true, m.FT, s[L_M2B], m.B1, s[L_M2A], Q);
    dw(L_M2A, m.H1, s[L_M1B], nullptr, 0, 0, m.B1, s[L_M2A], true);
    dw(L_ATC, m.C2, s[L_ATB], nullptr, 0, 0, m.SC, 1, true);
    dx(L_ATC, true, m.SC, 1, m.C2, s[L_ATB], Q);
    dw(L_ATB, m.C1, s[L_ATA], nullptr, 0, 0, m.C2, s[L_ATB], true);
    dx(L_ATB, true, m.C2, s[L_ATB], m.C1, s[L_ATA], Q);
    dw(L_ATA, m.H1, s[L_M1B], m.GQ, s[L_M1B], D.global ? H : 0, m.C1, s[L_ATA], true);
    dx(L_M2A, false, m.B1, s[L_M2A], m.D2, s[L_M1B], Q);
    dx(L_ATA, false, m.C1, s[L_ATA], m.D4, m.d4s, Q);
    hipLaunchKernelGGL(ebc::layers_h1_back, dim3(blocks_of((long long)Bp * H, 256)), dim3(256), 0, st, m.D2, s[L_M1B], m.D4, m.d4s, H, R,
                       D.global, m.N, Bp, m.H1, s[L_M1B]);
    dw(L_M1B, m.A1, s[L_M1A], nullptr, 0, 0, m.H1, s[L_M1B], true);
    dx(L_M1B, true, m.H1, s[L_M1B], m.A1, s[L_M1A], Q);
    dw(L_M1A, rows, T, nullptr, 0, 0, m.A1, s[L_M1A], true);
    HIP_TRY(hipGetLastError());
  }
  return EBC_OK;
}

}  // namespace

extern "C" int ebc_sarl_net_create_layers(const EbcSarlNetWeights *weights, int om_width, int device_id, void **net_out) {
  const std::string who = "ebc_sarl_net_create_layers: ";
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
  const int bad = grad_dims_refused_layers(widths, w.self_state_dim, om_width);
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
  if (bad == L_ATC + 2 || bad == L_M3D + 2)
    return fail(EBC_ERR_UNSUPPORTED, who + "the last layer of " + std::string(bad == L_ATC + 2 ? "attention" : "mlp3") + " has " +
                                         std::to_string(widths[bad - 1]) + " outputs, the gradient takes exactly 1");
  if (bad)
    return fail(EBC_ERR_UNSUPPORTED, who + "layer " + std::to_string(bad - 1) + " (counted through mlp1, mlp2, attention, mlp3) has " +
                                         std::to_string(widths[bad - 1]) + " units, the layer form takes 1 .. " +
                                         std::to_string(EBC_SARL_GRAD_LAYERS_MAX_WIDTH));
  for (int l = 0; l < EBC_SARL_GRAD_LAYERS; ++l)
    if (!w.weight[l] || !w.bias[l]) return fail(EBC_ERR_INVALID, who + "null weight or bias of layer " + std::to_string(l + 1));
  HIP_TRY(hipSetDevice(device_id));
  SarlNet *n = new SarlNet;
  n->device = device_id;
  widths[0] += om_width;  // the rows the gradient reads: the rotated columns, then the map
  n->D = grad_dims(widths, w.self_state_dim, w.with_global_state);
  n->max_rows = EBC_SARL_GRAD_LAYERS_MAX_ROWS;  // no passes: ebc_sarl_net_grad_max_rows_at refuses 4, 2, 1
  n->layers_grad = layers_grad;
  std::vector<float> image(n->D.floats);
  grad_pack(n->D, w.weight, w.bias, image.data());
  return ebc_host::grad_net_upload(n, image, "ebc_sarl_net_create_layers", net_out);
}
