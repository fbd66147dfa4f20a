// ebcsim_sail_grad.hip — training the SAIL network: ebc_sail_grad (the fused forward + backward kernel and the reduction
// of its chunk partials, ebc_sail_grad.h) and the packed image's accessors ebc_sail_packed_floats / _get_packed /
// _set_packed.  Its own translation unit: the forward's unit and the step kernels keep their code.
#include <hip/hip_runtime.h>

#include "ebc_grad_host.h"
#include "ebc_sail_api.h"
#include "ebc_sail_grad.h"

namespace {

using ebc_host::capturing;
using ebc_host::fail;

constexpr int kMaxChunksPerLaunch = 1024;  // 1024 chunks of partials (204 MB at 5 adults) before the float64 sums take over

}  // namespace

extern "C" int ebc_sail_grad(void *sail, void *stream, const EbcSailGradArgs *args) {
  if (!sail) return fail(EBC_ERR_INVALID, "null handle");
  if (!args || args->struct_size != sizeof(EbcSailGradArgs)) return fail(EBC_ERR_INVALID, "EbcSailGradArgs.struct_size");
  if (!args->grad || !args->loss_sum || !args->count || args->E < 0) return fail(EBC_ERR_INVALID, "ebc_sail_grad: grad, loss_sum, count, E");
  if (args->E > 0 && (!args->robot || !args->ob || !args->target)) return fail(EBC_ERR_INVALID, "ebc_sail_grad: robot, ob, target");
  const ebc_sail_api::View v = ebc_sail_api::view(sail);
  const int N = v.N, E = args->E;
  if (args->R < N)
    return fail(EBC_ERR_INVALID, "ebc_sail_grad: R < adult_num (row stride " + std::to_string(args->R) + ", adult_num " + std::to_string(N) + ")");
  if (capturing(stream))
    return fail(EBC_ERR_UNSUPPORTED, "ebc_sail_grad: the stream is being captured into a HIP graph; the gradient must be launched, not replayed");
  HIP_TRY(hipSetDevice(v.device));
  const hipStream_t st = (hipStream_t)stream;
  const int G = ebc_sail::grad_group_envs(N);
  const size_t lds = ebc::sail_grad_lds_floats(G, N) * sizeof(float);  // <= 110 KB
  static size_t raised_dev[64] = {0};
  HIP_TRY(ebc_host::raise_dynamic_lds(ebc::sail_grad_kernel, v.device, lds, raised_dev));
  ebc::SailGradLaunch a;
  a.robot = args->robot;
  a.ob = args->ob;
  a.n_rows = reinterpret_cast<const long long *>(args->n_rows);
  a.target = args->target;
  a.mask = args->sample_mask;
  a.action = args->action;
  a.grad_scale = args->grad_scale;
  a.E = E;
  a.R = args->R;
  a.N = N;
  const auto scratch = [sail](size_t bytes, void **out) { return ebc_sail_api::grad_scratch(sail, bytes, out); };  // the Sail object's own
  const auto launch = [&](int chunk0, int now, float *partial, double *loss_part, long long *count_part) {
    a.partial = partial, a.loss_part = loss_part, a.count_part = count_part, a.chunk0 = chunk0;
    hipLaunchKernelGGL(ebc::sail_grad_kernel, dim3((unsigned)now), dim3(64 * EBC_SAIL_GRAD_WAVES), lds, st, v.P, a);
  };
  return ebc_host::grad_launch<false>(st, ebc_sail::packed_floats(N), E, EBC_SAIL_GRAD_CHUNK, kMaxChunksPerLaunch, scratch, args->grad,
                                      args->loss_sum, args->count, launch);
}

extern "C" int ebc_sail_packed_floats(void *sail, int64_t *floats_out) {
  if (!sail || !floats_out) return fail(EBC_ERR_INVALID, "ebc_sail_packed_floats: null argument");
  *floats_out = (int64_t)ebc_sail::packed_floats(ebc_sail_api::view(sail).N);
  return EBC_OK;
}

extern "C" int ebc_sail_get_packed(void *sail, void *stream, float *dst_dev) {
  if (!sail || !dst_dev) return fail(EBC_ERR_INVALID, "ebc_sail_get_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_sail_get_packed: the stream is being captured into a HIP graph");
  const ebc_sail_api::View v = ebc_sail_api::view(sail);
  HIP_TRY(hipSetDevice(v.device));
  HIP_TRY(hipMemcpyAsync(dst_dev, v.P, ebc_sail::packed_floats(v.N) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

extern "C" int ebc_sail_set_packed(void *sail, void *stream, const float *src_dev) {
  if (!sail || !src_dev) return fail(EBC_ERR_INVALID, "ebc_sail_set_packed: null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, "ebc_sail_set_packed: the stream is being captured into a HIP graph");
  const ebc_sail_api::View v = ebc_sail_api::view(sail);
  HIP_TRY(hipSetDevice(v.device));
  // the image is the network's own device memory; View hands it out read-only to the kernels' launchers
  HIP_TRY(hipMemcpyAsync(const_cast<float *>(v.P), src_dev, ebc_sail::packed_floats(v.N) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}
