// ebcsim_cadrl.hip — the decision of the CADRL policy (rl/policy/cadrl.py:194-217): ebc_cadrl_decide.  Its own
// translation unit beside the simulation path, the two-layer blocks and the LSTM scan.
#include <hip/hip_runtime.h>

#include "ebc_cadrl.h"
#include "ebc_host.h"

using ebc_host::fail;

extern "C" int ebc_cadrl_decide(void *stream, const EbcCadrlArgs *args) {
  if (!args || args->struct_size != sizeof(EbcCadrlArgs)) return fail(EBC_ERR_INVALID, "EbcCadrlArgs.struct_size");
  if (!args->v || !args->reward || !args->values || !args->choice || args->E < 0)
    return fail(EBC_ERR_INVALID, "ebc_cadrl_decide: v, reward, values, choice, E");
  if (args->A < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_decide: A < 1 actions (" + std::to_string(args->A) + ")");
  if (args->R < 1) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_decide: R < 1 row slots per action (" + std::to_string(args->R) + ")");
  if (args->A > EBC_CADRL_MAX_ACTIONS) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_decide: A > 128 actions (" + std::to_string(args->A) + ")");
  if (args->R > EBC_CADRL_MAX_ROWS) return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_decide: R > 128 row slots per action (" + std::to_string(args->R) + ")");
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return fail(EBC_ERR_UNSUPPORTED, "ebc_cadrl_decide: the stream is being captured into a HIP graph; the decision must be launched, not replayed");
  if (args->E == 0) return EBC_OK;
  ebc::CadrlLaunch a;
  a.v = args->v;
  a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
  a.reward = args->reward;
  a.values = args->values;
  a.choice = args->choice;
  a.discount = args->discount;
  a.A = args->A;
  a.R = args->R;
  const size_t lds = (size_t)64 * (args->R | 1) * sizeof(float);  // <= 33 KB at R = 128
  hipLaunchKernelGGL(ebc::cadrl_decide_kernel, dim3((unsigned)args->E), dim3(64), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}
