// ebcsim_sail.hip — the SAIL policy's network and decision (rl/policy/sail.py): ebc_sail_create / _forward / _destroy.
// Its own translation unit beside the simulation path and the value-network units.
#include <hip/hip_runtime.h>

#include <vector>

#include "ebc_host.h"
#define EBC_SAIL_KERNEL  // this unit owns sail_kernel
#include "ebc_sail.h"
#include "ebc_sail_api.h"

namespace {

using ebc_host::fail;

struct Sail {
  int device = 0, N = 0;
  float *P = nullptr;
  void *grad_scratch = nullptr;  // ebc_sail_grad's chunk partials, grown on demand
  size_t grad_scratch_bytes = 0;
};

}  // namespace

ebc_sail_api::View ebc_sail_api::view(void *sail) {
  const Sail *s = static_cast<const Sail *>(sail);
  return View{s->P, s->N, s->device};
}

int ebc_sail_api::grad_scratch(void *sail, size_t bytes, void **out) {
  Sail *s = static_cast<Sail *>(sail);
  if (bytes > s->grad_scratch_bytes) {
    (void)hipFree(s->grad_scratch);  // waits for the work that may still read it
    s->grad_scratch = nullptr;
    s->grad_scratch_bytes = 0;
    if (hipMalloc(&s->grad_scratch, bytes) != hipSuccess) {
      s->grad_scratch = nullptr;
      return fail(EBC_ERR_DEVICE, "ebc_sail_grad: scratch allocation of " + std::to_string(bytes) + " bytes failed");
    }
    s->grad_scratch_bytes = bytes;
  }
  *out = s->grad_scratch;
  return EBC_OK;
}

int ebc_sail_api::launch(const float *P, int N, hipStream_t stream, const double *robot, const double *ob, const long long *n_rows,
                         double *action, float *feat_joint, int E, int R) {
  ebc::SailLaunch a;
  a.robot = robot;
  a.ob = ob;
  a.n_rows = n_rows;
  a.action = action;
  a.feat_joint = feat_joint;
  a.E = E;
  a.R = R;
  a.N = N;
  const int G = ebc_sail::group_envs(N);
  const size_t lds = ebc::sail_lds_floats(N) * sizeof(float);  // <= 48 KB
  hipLaunchKernelGGL(ebc::sail_kernel, dim3((unsigned)(((long long)E + G - 1) / G)), dim3(64 * EBC_SAIL_WAVES), lds, stream, P, a);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}

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
  return ebc_sail_api::launch(s->P, s->N, (hipStream_t)stream, args->robot, args->ob, reinterpret_cast<const long long *>(args->n_rows),
                              args->action, args->feat_joint, args->E, args->R);
}

extern "C" int ebc_sail_destroy(void *sail) {
  Sail *s = static_cast<Sail *>(sail);
  if (!s) return EBC_OK;
  (void)hipSetDevice(s->device);
  (void)hipFree(s->P);
  (void)hipFree(s->grad_scratch);
  delete s;
  return EBC_OK;
}
