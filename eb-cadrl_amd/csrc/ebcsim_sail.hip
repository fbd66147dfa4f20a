// ebcsim_sail.hip — the SAIL policy's network and decision (rl/policy/sail.py): ebc_sail_create / _forward / _destroy.
// Its own translation unit beside the simulation path and the value-network units.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_host.h"
#include "ebc_sail.h"

namespace {

using ebc_host::fail;

struct Sail {
  int device = 0, N = 0;
  float *P = nullptr;
};

}  // namespace

extern "C" int ebc_sail_create(const EbcSailWeights *w, int device_id, void **sail_out) {
  if (!w || !sail_out) return fail(EBC_ERR_INVALID, "ebc_sail_create: null argument");
  if (w->struct_size != sizeof(EbcSailWeights)) return fail(EBC_ERR_INVALID, "EbcSailWeights.struct_size");
  const int N = w->adult_num;
  if (N < EBC_SAIL_MIN_ADULTS)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sail: adult_num < 2 (" + std::to_string(N) + "): the reference's own transform_frame cannot reshape an empty selection");
  if (N > EBC_SAIL_MAX_ADULTS) return fail(EBC_ERR_UNSUPPORTED, "ebc_sail: adult_num > 32 (" + std::to_string(N) + ")");
  for (int l = 0; l < EBC_SAIL_LAYERS; ++l)
    if (!w->weight[l] || !w->bias[l]) return fail(EBC_ERR_INVALID, "ebc_sail_create: null weight or bias of layer " + std::to_string(l));
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(EBC_ERR_DEVICE, "no HIP device: libebcsim has no CPU fallback");
  if (device_id < 0 || device_id >= count) return fail(EBC_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  std::vector<float> P(ebc_sail::packed_floats(N));
  ebc_sail::pack(N, w->weight, w->bias, P.data());
  Sail *s = new Sail;
  s->device = device_id;
  s->N = N;
  if (hipMalloc(&s->P, P.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(s->P, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(s->P);
    delete s;
    return fail(EBC_ERR_DEVICE, "ebc_sail_create: device allocation or copy failed");
  }
  *sail_out = s;
  return EBC_OK;
}

extern "C" int ebc_sail_forward(void *sail, void *stream, const EbcSailArgs *args) {
  Sail *s = static_cast<Sail *>(sail);
  if (!s) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcSailArgs)) return fail(EBC_ERR_INVALID, "EbcSailArgs.struct_size");
  if (!args->robot || !args->ob || !args->action || args->E < 0) return fail(EBC_ERR_INVALID, "ebc_sail_forward: robot, ob, action, E");
  if (args->R < s->N)
    return fail(EBC_ERR_INVALID, "ebc_sail_forward: R < adult_num (row stride " + std::to_string(args->R) + ", adult_num " + std::to_string(s->N) + ")");
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sail_forward: the stream is being captured into a HIP graph; the forward must be launched, not replayed");
  if (args->E == 0) return EBC_OK;
  HIP_TRY(hipSetDevice(s->device));
  ebc::SailLaunch a;
  a.robot = args->robot;
  a.ob = args->ob;
  a.n_rows = reinterpret_cast<const long long *>(args->n_rows);
  a.action = args->action;
  a.feat_joint = args->feat_joint;
  a.E = args->E;
  a.R = args->R;
  a.N = s->N;
  const int G = ebc_sail::group_envs(s->N);
  const size_t lds = ebc::sail_lds_floats(s->N) * sizeof(float);  // <= 48 KB
  hipLaunchKernelGGL(ebc::sail_kernel, dim3((unsigned)(((long long)args->E + G - 1) / G)), dim3(64 * EBC_SAIL_WAVES), lds, (hipStream_t)stream,
                     s->P, a);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

extern "C" int ebc_sail_destroy(void *sail) {
  Sail *s = static_cast<Sail *>(sail);
  if (!s) return EBC_OK;
  (void)hipSetDevice(s->device);
  (void)hipFree(s->P);
  delete s;
  return EBC_OK;
}
