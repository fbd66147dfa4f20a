// ebcsim_vn_wide.hip — the wide two-layer value-network blocks of libebcsim.so (ebc_mlp2_create_wide handles): a
// translation unit of its own, compiled beside the others.  Kernels and the entries' declarations: ebc_vn_wide.h; the
// handle, its packing and the C entries: ebcsim_value_net.hip.
#include <hip/hip_runtime.h>

#include <map>

#include "ebc_vn_wide.h"

using ebc_host::fail;

namespace {

struct WideState {
  struct Buf {
    void *ptr = nullptr;
    size_t bytes = 0;
  };
  std::map<hipStream_t, Buf> scratch;  // the hidden layer of the launches in flight on a stream
};

// The stream's scratch with room for `bytes`, and layer 1's LDS limit raised on this device (lds: 0 = nothing to raise).
// Either may allocate or change a function attribute, which a stream under capture cannot take.
template <class Kernel>
int prepare(WideState *ws, int device, hipStream_t st, size_t bytes, Kernel *kernel, size_t lds, size_t (&raised)[64], void **out) {
  WideState::Buf &b = ws->scratch[st];
  const bool grow = b.bytes < bytes, raise = lds > 65536 && raised[device & 63] < lds;
  if ((grow || raise) && ebc_host::capturing(st))
    return fail(EBC_ERR_UNSUPPORTED, "wide mlp2 block: this call has to allocate its hidden-layer scratch or raise an LDS limit, "
                                     "which a stream under capture cannot do: run it once outside the capture");
  if (raise) HIP_TRY(ebc_host::raise_dynamic_lds(kernel, device, lds, raised));
  if (grow) {
    if (b.ptr) HIP_TRY(hipFree(b.ptr));  // (waits for the launches that still read it)
    b.ptr = nullptr;
    b.bytes = 0;
    HIP_TRY(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
  }
  *out = b.ptr;
  return EBC_OK;
}

}  // namespace

namespace ebc_host {

void *vn_wide_state_new() { return new WideState(); }

void vn_wide_state_free(void *state) {
  WideState *ws = (WideState *)state;
  if (!ws) return;
  for (auto &kv : ws->scratch)
    if (kv.second.ptr) (void)hipFree(kv.second.ptr);
  delete ws;
}

int vn_wide_forward(void *state, const VnWideCall &c, const ebc::PackedLayer &L1, const ebc::PackedLayer &L2) {
#ifdef EBC_DEV_GS
  return fail(EBC_ERR_UNSUPPORTED, "development build: no value-network blocks");
#else
  WideState *ws = (WideState *)state;
  const int slab = c.M < EBC_VNW_SLAB ? c.M : EBC_VNW_SLAB;
  const size_t bytes = (size_t)((slab + 31) / 32) * L1.out_tiles * 4096;
  static size_t raised[64] = {0};
  void *hid = nullptr;
  const size_t lds1 = ebc::vnw_lds_bytes(true), lds2 = ebc::vnw_lds_bytes(false);
  static_assert(ebc::vnw_lds_bytes(false) <= 65536, "layer 2 runs within the default LDS limit");
  const int rc = prepare(ws, c.device, c.st, bytes, ebc::wide_layer_kernel<true>, lds1, raised, &hid);
  if (rc != EBC_OK) return rc;
  const int passes1 = (L1.out_tiles + EBC_VNW_TG - 1) / EBC_VNW_TG, passes2 = (L2.out_tiles + EBC_VNW_TG - 1) / EBC_VNW_TG;
  for (int r0 = 0; r0 < c.M; r0 += EBC_VNW_SLAB) {
    const int rows = c.M - r0 < EBC_VNW_SLAB ? c.M - r0 : EBC_VNW_SLAB;
    const unsigned wgs = (unsigned)((rows + EBC_VNW_ROWS - 1) / EBC_VNW_ROWS);
    ebc::WideArgs a1 = {c.x + (size_t)r0 * c.K0, nullptr, (uint4 *)hid, nullptr, rows, c.K0, c.H, r0, c.row_bias, c.group_rows, nullptr, 0.0f, 1};
    hipLaunchKernelGGL((ebc::wide_layer_kernel<true>), dim3(wgs, (unsigned)passes1), dim3(64 * EBC_VNW_NW), lds1, c.st, L1, a1);
    HIP_TRY(hipGetLastError());
    // the tail's dot product crosses the passes: one workgroup walks them in order
    float *y = c.y + (size_t)r0 * (c.final_w ? 1 : c.O);
    ebc::WideArgs a2 = {nullptr, (const uint4 *)hid, nullptr, y, rows, c.H, c.O, r0, nullptr, 0, c.final_w, c.final_b, c.relu_out};
    hipLaunchKernelGGL((ebc::wide_layer_kernel<false>), dim3(wgs, (unsigned)(c.final_w ? 1 : passes2)), dim3(64 * EBC_VNW_NW), lds2, c.st, L2, a2);
    HIP_TRY(hipGetLastError());
  }
  return EBC_OK;
#endif
}

int vn_wide_forward_f32(void *state, const VnWideCall &c, const ebc::WideF32Layer &F1, const ebc::WideF32Layer &F2) {
#ifdef EBC_DEV_GS
  return fail(EBC_ERR_UNSUPPORTED, "development build: no value-network blocks");
#else
  WideState *ws = (WideState *)state;
  const int slab = c.M < EBC_VNW_SLAB ? c.M : EBC_VNW_SLAB;
  static size_t raised[64] = {0};
  void *hid = nullptr;
  const int rc = prepare(ws, c.device, c.st, (size_t)slab * c.H * 4, ebc::wide_f32_layer_kernel<true>, 0, raised, &hid);
  if (rc != EBC_OK) return rc;
  for (int r0 = 0; r0 < c.M; r0 += EBC_VNW_SLAB) {
    const int rows = c.M - r0 < EBC_VNW_SLAB ? c.M - r0 : EBC_VNW_SLAB;
    const dim3 grid((unsigned)((rows + 31) / 32)), block(256);
    ebc::WideArgs a1 = {c.x + (size_t)r0 * c.K0, nullptr, nullptr, (float *)hid, rows, c.K0, c.H, r0, c.row_bias, c.group_rows, nullptr, 0.0f, 1};
    hipLaunchKernelGGL((ebc::wide_f32_layer_kernel<true>), grid, block, 0, c.st, F1, a1);
    HIP_TRY(hipGetLastError());
    float *y = c.y + (size_t)r0 * (c.final_w ? 1 : c.O);
    ebc::WideArgs a2 = {(const float *)hid, nullptr, nullptr, y, rows, c.H, c.O, r0, nullptr, 0, c.final_w, c.final_b, c.relu_out};
    hipLaunchKernelGGL((ebc::wide_f32_layer_kernel<false>), grid, block, 0, c.st, F2, a2);
    HIP_TRY(hipGetLastError());
  }
  return EBC_OK;
#endif
}

}  // namespace ebc_host
