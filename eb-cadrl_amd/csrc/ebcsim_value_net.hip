// ebcsim_value_net.hip — the value-network blocks of libebcsim.so (ebc_mlp2_* / ebc_pair_*): a translation unit of
// its own, compiled beside ebcsim.hip.  Kernels: ebc_value_net.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ebc_host.h"
#include "ebc_value_net.h"
#include "ebc_vn_stream_api.h"
#include "ebc_vn_wide.h"

using ebc_host::fail;

// ------------------------------------------------------------------------- value-network layers
namespace {

uint16_t bf16_rn(float v) {  // round to nearest even, as v_cvt_pk_bf16_f32
  uint32_t u;
  memcpy(&u, &v, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16);  // inf / nan
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf16_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float v;
  memcpy(&v, &u, 4);
  return v;
}

struct Mlp2 {
  int device = 0, K0 = 0, H = 0, O = 0;
  ebc::PackedLayer L1{}, L2{};
  ebc::F32Layer F1{}, F2{};  // the same weights transposed in float32 (ebc_mlp2_forward_f32)
  int in_frag = 0;           // EBC_MLP_IN_FRAGMENTS: the first layer packed in accumulator k order (input = fragments)
  float *final_w = nullptr;  // optional third layer with one output
  float final_b = 0.0f;
  void *wide = nullptr;      // ebc_mlp2_create_wide: the block runs on the single-layer kernels of ebc_vn_wide.h (its scratch)
  std::vector<void *> allocs;
};

// W [out][in] (torch Linear layout) -> A fragments of mfma_f32_32x32x16_bf16, split in hi / lo.
// acc_order: the layer's input is an accumulator tile of the layer before (fragment element j of lane
// half h in k-step s is row 16 s + 8 (j >> 2) + 4 h + (j & 3)); otherwise natural order 16 s + 8 h + j.
int pack_layer(Mlp2 *m, const float *W, const float *b, int out, int in, bool acc_order, ebc::PackedLayer *L) {
  const int To = (out + 31) / 32, Ti = (in + 31) / 32;
  std::vector<uint16_t> frag((size_t)To * Ti * 2 * 2 * 64 * 8);
  for (int t = 0; t < To; ++t)
    for (int u = 0; u < Ti; ++u)
      for (int s = 0; s < 2; ++s)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int i = lane & 31, hh = lane >> 5;
            const int k = acc_order ? 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3) : 16 * s + 8 * hh + j;
            const int row = t * 32 + i, colk = u * 32 + k;
            const float v = (row < out && colk < in) ? W[(size_t)row * in + colk] : 0.0f;
            const uint16_t hi = bf16_rn(v), lo = bf16_rn(v - bf16_to_float(hi));
            const size_t base = ((((size_t)t * Ti + u) * 2 + s) * 2) * 64 * 8;
            frag[base + (size_t)lane * 8 + j] = hi;
            frag[base + 64 * 8 + (size_t)lane * 8 + j] = lo;
          }
  std::vector<float> bias((size_t)To * 2 * 16, 0.0f);
  for (int t = 0; t < To; ++t)
    for (int hh = 0; hh < 2; ++hh)
      for (int r = 0; r < 16; ++r) {
        const int unit = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (unit < out) bias[((size_t)t * 2 + hh) * 16 + r] = b[unit];
      }
  void *df = nullptr, *db = nullptr;
  HIP_TRY(hipMalloc(&df, frag.size() * 2));
  m->allocs.push_back(df);
  HIP_TRY(hipMalloc(&db, bias.size() * 4));
  m->allocs.push_back(db);
  HIP_TRY(hipMemcpy(df, frag.data(), frag.size() * 2, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(db, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
  L->frag = (const uint4 *)df;
  L->bias = (const float *)db;
  L->in_tiles = Ti;
  L->out_tiles = To;
  return EBC_OK;
}

// W [out][in] -> transposed [in][out padded to 64], float32 as it is
int pack_f32(Mlp2 *m, const float *W, const float *b, int out, int in, ebc::F32Layer *L) {
  const int out_pad = (out + 63) / 64 * 64;
  if (!m->wide && out_pad > 64 * EBC_F32_MAXU) return fail(EBC_ERR_UNSUPPORTED, "mlp2: more than 320 units in a layer");
  std::vector<float> wt((size_t)in * out_pad, 0.0f), bias((size_t)out_pad, 0.0f);
  for (int o = 0; o < out; ++o) {
    bias[o] = b[o];
    for (int k = 0; k < in; ++k) wt[(size_t)k * out_pad + o] = W[(size_t)o * in + k];
  }
  void *dw = nullptr, *db = nullptr;
  HIP_TRY(hipMalloc(&dw, wt.size() * 4));
  m->allocs.push_back(dw);
  HIP_TRY(hipMalloc(&db, bias.size() * 4));
  m->allocs.push_back(db);
  HIP_TRY(hipMemcpy(dw, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(db, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
  L->wt = (const float *)dw;
  L->b = (const float *)db;
  L->in = in;
  L->out = out;
  L->out_pad = out_pad;
  return EBC_OK;
}

// One (TI, TO, GROUP, KIN) = one kernel: the waves per workgroup, the LDS layout and its bytes are VnLayout's
// (ebc_vn_layout.h), which the kernel reads too.
template <int TI, int TO, bool GROUP, int KIN>
int launch_mlp2_kernel(const Mlp2 *m, hipStream_t st, const float *x, int M, int relu_out, float *y, const ebc::MlpExtra &ex) {
  constexpr ebc::VnLayout ly{TI, TO};
  const size_t lds = ly.lds_bytes(m->L1.out_tiles, GROUP);
  static size_t raised[64] = {0};
  HIP_TRY(ebc_host::raise_dynamic_lds(ebc::mlp2_split_wg_kernel<TI, TO, GROUP, KIN>, m->device, lds, raised));
  constexpr int rows = 32 * ly.nw();
  const dim3 grid((unsigned)((M + rows - 1) / rows)), block(64 * ly.nw());
  hipLaunchKernelGGL((ebc::mlp2_split_wg_kernel<TI, TO, GROUP, KIN>), grid, block, lds, st, x, M, m->K0, m->L1, m->L2, relu_out, y, m->O, ex);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

template <int TI, int TO>
int launch_mlp2_to(const Mlp2 *m, hipStream_t st, const float *x, int M, int relu_out, float *y, const ebc::MlpExtra &ex) {
  // the row-group sums live in the coalesced-output epilogue (ebc_value_net.h): the block must be one that takes it
  if (ex.partial && !ebc::VnLayout{TI, TO}.has_tile_epilogue(m->O))
    return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_reduce: this block shape has no tile epilogue");
  // 200-wide inputs (the h1 rows of mlp2 and of the attention stack) end in the first half of their seventh tile
  if constexpr (TI == 7) {
    if (m->K0 <= 32 * TI - 16)
      return ex.row_bias ? launch_mlp2_kernel<TI, TO, true, 1>(m, st, x, M, relu_out, y, ex) : launch_mlp2_kernel<TI, TO, false, 1>(m, st, x, M, relu_out, y, ex);
  }
  return ex.row_bias ? launch_mlp2_kernel<TI, TO, true, 0>(m, st, x, M, relu_out, y, ex) : launch_mlp2_kernel<TI, TO, false, 0>(m, st, x, M, relu_out, y, ex);
}

template <int TI>
int launch_mlp2(const Mlp2 *m, hipStream_t st, const float *x, int M, int relu_out, float *y, const ebc::MlpExtra &ex) {
  switch (m->L2.out_tiles) {
    case 1: return launch_mlp2_to<TI, 1>(m, st, x, M, relu_out, y, ex);
    case 2: return launch_mlp2_to<TI, 2>(m, st, x, M, relu_out, y, ex);
    case 3: return launch_mlp2_to<TI, 3>(m, st, x, M, relu_out, y, ex);
    case 4: return launch_mlp2_to<TI, 4>(m, st, x, M, relu_out, y, ex);
    case 5: return launch_mlp2_to<TI, 5>(m, st, x, M, relu_out, y, ex);
    case 6: return launch_mlp2_to<TI, 6>(m, st, x, M, relu_out, y, ex);
    case 7: return launch_mlp2_to<TI, 7>(m, st, x, M, relu_out, y, ex);
    default: return fail(EBC_ERR_UNSUPPORTED, "mlp2: more than 224 outputs");
  }
}

int mlp2_dispatch(const Mlp2 *m, hipStream_t st, const float *x, int M, int relu_out, float *y, const ebc::MlpExtra &ex) {
#ifdef EBC_DEV_GS
  return fail(EBC_ERR_UNSUPPORTED, "development build: no value-network blocks");
#else
  switch (m->L1.in_tiles) {
    case 1: return launch_mlp2<1>(m, st, x, M, relu_out, y, ex);
    case 2: return launch_mlp2<2>(m, st, x, M, relu_out, y, ex);
    case 3: return launch_mlp2<3>(m, st, x, M, relu_out, y, ex);
    case 4: return launch_mlp2<4>(m, st, x, M, relu_out, y, ex);
    case 5: return launch_mlp2<5>(m, st, x, M, relu_out, y, ex);
    case 6: return launch_mlp2<6>(m, st, x, M, relu_out, y, ex);
    default: return launch_mlp2<7>(m, st, x, M, relu_out, y, ex);
  }
#endif
}

ebc_host::VnWideCall wide_call(const Mlp2 *m, hipStream_t st, const float *x, int M, int relu_out, const float *row_bias, int group_rows,
                               float *y) {
  return {m->device, st, m->K0, m->H, m->O, M, relu_out, x, row_bias, group_rows, m->final_w, m->final_b, y};
}

}  // namespace

extern "C" {

int ebc_mlp2_create(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2,
                    const float *b2, const float *w3, const float *b3, void **out) {
  return ebc_mlp2_create_ex(device_id, K0, H, O, w1, b1, w2, b2, w3, b3, 0, out);
}

static int mlp2_create(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2, const float *b2,
                       const float *w3, const float *b3, int flags, bool wide, void **out);

int ebc_mlp2_create_ex(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *w3, const float *b3, int flags, void **out) {
  if (!w1 || !b1 || !w2 || !b2 || !out) return fail(EBC_ERR_INVALID, "null argument");
  if (K0 <= 0 || H <= 0 || O <= 0 || K0 > 224 || O > 224 || H > 320) return fail(EBC_ERR_UNSUPPORTED, "mlp2 dimensions");
  return mlp2_create(device_id, K0, H, O, w1, b1, w2, b2, w3, b3, flags, false, out);
}

int ebc_mlp2_create_wide(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2,
                         const float *b2, const float *w3, const float *b3, int flags, void **out) {
  if (!w1 || !b1 || !w2 || !b2 || !out) return fail(EBC_ERR_INVALID, "null argument");
  if (K0 < 1 || H < 1 || O < 1 || K0 > EBC_VNW_MAX || H > EBC_VNW_MAX || O > EBC_VNW_MAX)
    return fail(EBC_ERR_UNSUPPORTED, "wide mlp2 block: K0, H and O must each lie in 1 .. 640");
  if (flags & EBC_MLP_IN_FRAGMENTS) return fail(EBC_ERR_UNSUPPORTED, "wide mlp2 block: EBC_MLP_IN_FRAGMENTS is not taken (rows in, rows out)");
  if (flags) return fail(EBC_ERR_INVALID, "wide mlp2 block: unknown flags");
  return mlp2_create(device_id, K0, H, O, w1, b1, w2, b2, w3, b3, 0, true, out);
}

static int mlp2_create(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2, const float *b2,
                       const float *w3, const float *b3, int flags, bool wide, void **out) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(EBC_ERR_DEVICE, "no HIP device: libebcsim has no CPU fallback");
  if (device_id < 0 || device_id >= count) return fail(EBC_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  Mlp2 *m = new Mlp2();
  m->device = device_id; m->K0 = K0; m->H = H; m->O = O;
  m->in_frag = (flags & EBC_MLP_IN_FRAGMENTS) ? 1 : 0;
  if (wide) m->wide = ebc_host::vn_wide_state_new();
  int rc = pack_layer(m, w1, b1, H, K0, m->in_frag != 0, &m->L1);
  if (rc == EBC_OK) rc = pack_layer(m, w2, b2, O, H, true, &m->L2);
  if (rc == EBC_OK) rc = pack_f32(m, w1, b1, H, K0, &m->F1);
  if (rc == EBC_OK) rc = pack_f32(m, w2, b2, O, H, &m->F2);
  if (rc == EBC_OK && w3) {
    void *dw = nullptr;
    if (hipMalloc(&dw, (size_t)O * 4) != hipSuccess || hipMemcpy(dw, w3, (size_t)O * 4, hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(EBC_ERR_DEVICE, "mlp2: third layer upload failed");
    if (dw) m->allocs.push_back(dw);
    m->final_w = (float *)dw;
    m->final_b = b3 ? b3[0] : 0.0f;
  }
  if (rc != EBC_OK) {
    for (void *ptr : m->allocs) (void)hipFree(ptr);
    ebc_host::vn_wide_state_free(m->wide);
    delete m;
    return rc;
  }
  *out = m;
  return EBC_OK;
}

int ebc_mlp2_forward(void *mlp, void *stream, const float *x, int M, int relu_out, const float *row_bias,
                     int group_rows, float *y) {
  Mlp2 *m = (Mlp2 *)mlp;
  if (!m || !x || !y || M < 0) return fail(EBC_ERR_INVALID, "mlp2 forward arguments");
  if (row_bias && group_rows <= 0) return fail(EBC_ERR_INVALID, "mlp2: group_rows");
  if (M == 0) return EBC_OK;
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)stream;
  if (m->wide) return ebc_host::vn_wide_forward(m->wide, wide_call(m, st, x, M, relu_out, row_bias, group_rows, y), m->L1, m->L2);
  const ebc::MlpExtra ex = {row_bias, group_rows, m->H, m->final_w, m->final_b, nullptr, nullptr, 0, 1};
  return mlp2_dispatch(m, st, x, M, relu_out, y, ex);
}

int ebc_mlp2_update(void *mlp, void *stream, const float *w1, const float *b1, const float *w2, const float *b2,
                    const float *w3, const float *b3) {
  Mlp2 *m = (Mlp2 *)mlp;
  if (!m || !w1 || !b1 || !w2 || !b2) return fail(EBC_ERR_INVALID, "mlp2 update arguments");
  if ((m->final_w != nullptr) != (w3 != nullptr)) return fail(EBC_ERR_INVALID, "mlp2 update: third layer given / missing");
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)stream;
  struct { const float *W, *b; int out, in, acc; ebc::PackedLayer *L; ebc::F32Layer *F; } layers[2] = {
      {w1, b1, m->H, m->K0, m->in_frag, &m->L1, &m->F1}, {w2, b2, m->O, m->H, 1, &m->L2, &m->F2}};
  for (auto &l : layers) {
    const size_t To = (l.out + 31) / 32, Ti = (l.in + 31) / 32;
    size_t n = To * Ti * 2 * 64 * 8;
    if ((size_t)l.in * l.F->out_pad > n) n = (size_t)l.in * l.F->out_pad;
    hipLaunchKernelGGL(ebc::mlp2_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, l.W, l.b, l.out, l.in, l.acc,
                       (unsigned short *)const_cast<uint4 *>(l.L->frag), const_cast<float *>(l.L->bias),
                       const_cast<float *>(l.F->wt), const_cast<float *>(l.F->b), l.F->out_pad);
    HIP_TRY(hipGetLastError());
  }
  if (w3) {
    HIP_TRY(hipMemcpyAsync(m->final_w, w3, (size_t)m->O * 4, hipMemcpyDeviceToDevice, st));
    float fb = 0.0f;  // the one scalar of the block that lives in the handle: read back (a few bytes, once per update)
    if (b3) {
      HIP_TRY(hipMemcpyAsync(&fb, b3, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    m->final_b = fb;
  }
  return EBC_OK;
}

int ebc_mlp2_forward_f32(void *mlp, void *stream, const float *x, int M, int relu_out, const float *row_bias,
                         int group_rows, float *y) {
  Mlp2 *m = (Mlp2 *)mlp;
  if (!m || !x || !y || M < 0) return fail(EBC_ERR_INVALID, "mlp2 forward arguments");
  if (row_bias && group_rows <= 0) return fail(EBC_ERR_INVALID, "mlp2: group_rows");
  if (M == 0) return EBC_OK;
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)stream;
  if (m->wide) {
    const ebc::WideF32Layer f1 = {m->F1.wt, m->F1.b, m->F1.in, m->F1.out, m->F1.out_pad}, f2 = {m->F2.wt, m->F2.b, m->F2.in, m->F2.out, m->F2.out_pad};
    return ebc_host::vn_wide_forward_f32(m->wide, wide_call(m, st, x, M, relu_out, row_bias, group_rows, y), f1, f2);
  }
  // few rows: a workgroup per 32-row tile, its waves sharing the tile (the form a decision's re-evaluation gets); many
  // rows: four tiles per workgroup walking the hidden tiles together on weights staged in LDS.
  if (M <= EBC_F32_TILE_ROWS) {
    constexpr int NW = 8;
    const size_t tl = ((size_t)((m->K0 + 3) & ~3) * 32 + (size_t)((m->H + 31) / 32) * 1024 + NW * 32) * 4;
    static size_t raised_tile[64] = {0};
    HIP_TRY(ebc_host::raise_dynamic_lds(ebc::mlp2_f32_tile_kernel<NW>, m->device, tl, raised_tile));
    hipLaunchKernelGGL((ebc::mlp2_f32_tile_kernel<NW>), dim3((unsigned)((M + 31) / 32)), dim3(NW * 64), tl, st, x, M, m->F1, m->F2,
                       relu_out, y, row_bias, group_rows, (const float *)m->final_w, m->final_b);
    HIP_TRY(hipGetLastError());
    return EBC_OK;
  }
  const size_t lds = ((size_t)((m->K0 + 3) & ~3) * 32 + (size_t)32 * m->F2.out_pad) * 4;  // a hidden tile's W1 columns + W2 rows
  const dim3 grid((unsigned)((M + 127) / 128)), block(256);
  static size_t raised[8][64] = {{0}};  // per output-tile count: a kernel each
#define F32_(T2)                                                                                                         \
  HIP_TRY(ebc_host::raise_dynamic_lds(ebc::mlp2_f32_kernel<T2>, m->device, lds, raised[T2]));                            \
  hipLaunchKernelGGL((ebc::mlp2_f32_kernel<T2>), grid, block, lds, st, x, M, m->F1, m->F2, relu_out, y, row_bias, group_rows, \
                     (const float *)m->final_w, m->final_b)
  switch ((m->O + 31) / 32) {
    case 1: F32_(1); break;
    case 2: F32_(2); break;
    case 3: F32_(3); break;
    case 4: F32_(4); break;
    case 5: F32_(5); break;
    case 6: F32_(6); break;
    default: F32_(7); break;
  }
#undef F32_
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_mlp2_forward_reduce(void *mlp, void *stream, const float *x, int M, int relu_out, const float *row_bias,
                            int group_rows, float *y, int seg_rows, const float *row_weight, double *partial) {
  Mlp2 *m = (Mlp2 *)mlp;
  if (!m || !x || !partial || M < 0) return fail(EBC_ERR_INVALID, "mlp2 forward_reduce arguments");
  if (m->wide) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_reduce: a wide block has no tile epilogue (no partial sums)");
  if (row_bias && group_rows <= 0) return fail(EBC_ERR_INVALID, "mlp2: group_rows");
  if (m->final_w) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_reduce: a block with a one-output third layer has no [M][O] rows");
  if (seg_rows < 16) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_reduce: groups of fewer than 16 rows (a tile would touch more than three)");
  if (m->O & 3) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_reduce: O must be a multiple of 4");
  if (M == 0) return EBC_OK;
  HIP_TRY(hipSetDevice(m->device));
  const ebc::MlpExtra ex = {row_bias, group_rows, m->H, nullptr, 0.0f, row_weight, partial, seg_rows, y ? 1 : 0};
  return mlp2_dispatch(m, (hipStream_t)stream, x, M, relu_out, y, ex);
}

int ebc_mlp2_forward_ex(void *mlp, void *stream, const EbcMlpArgs *a) {
  Mlp2 *m = (Mlp2 *)mlp;
  if (!m || !a || a->struct_size != sizeof(EbcMlpArgs)) return fail(EBC_ERR_INVALID, "EbcMlpArgs.struct_size");
  if (a->M < 0 || (!a->x && !a->frag_in)) return fail(EBC_ERR_INVALID, "mlp2 forward_ex: no input");
  if (m->wide) {  // plain rows only, which is ebc_mlp2_forward
    if (a->frag_in || a->frag_out) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: a wide block takes and leaves rows, not fragments (frag_in / frag_out)");
    if (a->partial || a->seg_rows || a->row_weight)
      return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: a wide block has no tile epilogue (partial / seg_rows / row_weight)");
    if (a->flags & EBC_MLP_GENERAL_KERNEL) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: EBC_MLP_GENERAL_KERNEL on a wide block (it has one kernel)");
    if (!a->y) return fail(EBC_ERR_INVALID, "mlp2 forward_ex: no output");
    return ebc_mlp2_forward(mlp, stream, a->x, a->M, a->relu_out, a->row_bias, a->group_rows, a->y);
  }
  if ((a->frag_in != nullptr) != (m->in_frag != 0))
    return fail(EBC_ERR_INVALID, "mlp2 forward_ex: fragment input needs a block created with EBC_MLP_IN_FRAGMENTS, row input one without");
  if (a->row_bias && a->group_rows <= 0) return fail(EBC_ERR_INVALID, "mlp2: group_rows");
  if (a->partial) {
    if (m->final_w) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: a block with a one-output third layer has no [M][O] rows");
    if (a->seg_rows < 16) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: groups of fewer than 16 rows");
  }
  if ((a->partial || a->frag_out) && (m->O & 3)) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: O must be a multiple of 4");
  if (a->frag_out && m->final_w) return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: a one-output block has no tiles to hand on");
  if (!a->y && !a->partial && !a->frag_out) return fail(EBC_ERR_INVALID, "mlp2 forward_ex: no output");
  if (a->M == 0) return EBC_OK;
  HIP_TRY(hipSetDevice(m->device));
  // the tile epilogue writes rows only when asked to (store_y) once partial sums or fragments are wanted
  const int store_y = a->y ? 1 : 0;
  ebc::MlpExtra ex = {a->row_bias, a->group_rows, m->H, m->final_w, m->final_b, a->row_weight, a->partial, a->seg_rows, store_y,
                      (const uint4 *)a->frag_in, (uint4 *)a->frag_out};
  if (!a->partial && a->frag_out) {  // fragments without sums: the sums' machinery with nothing to add up to
    return fail(EBC_ERR_UNSUPPORTED, "mlp2 forward_ex: frag_out comes with partial sums (the tile epilogue)");
  }
  if (!(a->flags & EBC_MLP_GENERAL_KERNEL)) {  // the attention block at its widest: the streamed kernel (ebc_vn_stream.h)
    const int rc = ebc_host::vn_stream_launch(m->device, (hipStream_t)stream, a->M, m->L1, m->L2, m->K0, m->H, m->O, a->y, ex, a->relu_out, a->x);
    if (rc != EBC_VN_STREAM_NA) return rc;
  }
  return mlp2_dispatch(m, (hipStream_t)stream, a->x, a->M, a->relu_out, a->y, ex);
}

int ebc_pair_weights(void *stream, const float *scores, const long long *n_valid, int B, int R, float *w) {
  if (!scores || !w || B < 0 || R <= 0) return fail(EBC_ERR_INVALID, "pair_weights arguments");
  if (B == 0) return EBC_OK;
  hipLaunchKernelGGL(ebc::pair_weights_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores, n_valid, B, R, w);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_pair_mask(void *stream, const long long *n_valid, int B, int R, float *w) {
  if (!n_valid || !w || B < 0 || R <= 0) return fail(EBC_ERR_INVALID, "pair_mask arguments");
  if (B == 0) return EBC_OK;
  const size_t n = (size_t)B * R;
  hipLaunchKernelGGL(ebc::pair_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_valid, B, R, w);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_pair_combine(void *stream, const double *partial, const long long *n_valid, int B, int R, int O, int mean, float *out) {
  if (!partial || !out || B < 0 || R < 16 || R > 32 || O <= 0) return fail(EBC_ERR_INVALID, "pair_combine arguments (16 <= R <= 32)");
  if ((O & 3) || (((size_t)partial | (size_t)out) & 15)) return fail(EBC_ERR_INVALID, "pair_combine: O a multiple of 4, 16-byte aligned buffers");
  if (B == 0) return EBC_OK;
  hipLaunchKernelGGL(ebc::pair_combine_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, partial, n_valid, B, R, O,
                     mean, out);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_pair_mean(void *stream, const float *h, const long long *n_valid, int B, int R, int H, float *g) {
  if (!h || !g || B < 0 || R <= 0 || H <= 0) return fail(EBC_ERR_INVALID, "pair_mean arguments");
  if (B == 0) return EBC_OK;
  if (((size_t)h | (size_t)g) & 15 || (H & 3)) {
    if (H & 3) return fail(EBC_ERR_UNSUPPORTED, "pair_mean: H must be a multiple of 4");
    return fail(EBC_ERR_INVALID, "pair_mean: 16-byte aligned buffers");
  }
  hipLaunchKernelGGL(ebc::pair_mean_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, h, n_valid, B, R, H, g);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_pair_attend(void *stream, const float *scores, const float *feat, const long long *n_valid, int B, int R, int F,
                    float *out) {
  if (!scores || !feat || !out || B < 0 || R <= 0 || F <= 0) return fail(EBC_ERR_INVALID, "pair_attend arguments");
  if (B == 0) return EBC_OK;
  if ((F & 3) || F > 256) return fail(EBC_ERR_UNSUPPORTED, "pair_attend: F must be a multiple of 4, at most 256");
  if (((size_t)feat | (size_t)out) & 15) return fail(EBC_ERR_INVALID, "pair_attend: 16-byte aligned buffers");
  hipLaunchKernelGGL(ebc::pair_attend_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, scores, feat,
                     n_valid, B, R, F, out);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

int ebc_mlp2_destroy(void *mlp) {
  Mlp2 *m = (Mlp2 *)mlp;
  if (!m) return EBC_OK;
  for (void *ptr : m->allocs) (void)hipFree(ptr);
  ebc_host::vn_wide_state_free(m->wide);
  delete m;
  return EBC_OK;
}

}  // extern "C"

