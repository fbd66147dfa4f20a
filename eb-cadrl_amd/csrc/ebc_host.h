// ebc_host.h — host-side helpers shared by the translation units of libebcsim.so (ebcsim.hip: the simulation path;
// ebcsim_value_net.hip: the value-network blocks; ebcsim_vn_stream.hip: the streamed blocks — units that compile side
// by side).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ebcsim.h"

namespace ebc_host {

inline thread_local std::string g_err;  // ebc_last_error(): one per thread, shared by the units (C++17 inline variable)

inline int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

// A launch gets 64 KB of dynamic LDS by default; a kernel that needs more has that raised as a function attribute, which
// is per device: done when a launch asks for more than this kernel has on that device so far.
template <class Kernel>
hipError_t raise_dynamic_lds(Kernel *kernel, int device, size_t lds, size_t (&raised)[64]) {
  size_t &have = raised[device & 63];
  if (lds <= 65536 || lds <= have) return hipSuccess;
  const hipError_t err = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err == hipSuccess) have = lds;
  return err;
}

// a stream that is being captured into a HIP graph: the entries that allocate or copy outside the graph refuse it
inline bool capturing(void *stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

}  // namespace ebc_host

#define HIP_TRY(x)                                                                                    \
  do {                                                                                                \
    hipError_t err__ = (x);                                                                           \
    if (err__ != hipSuccess)                                                                          \
      return ebc_host::fail(EBC_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(err__));       \
  } while (0)
