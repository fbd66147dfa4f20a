// ebcsim_world.hip — ebc_step_k_world with EBC_FLAG_ONE_LAUNCH: the instantiations of the one-launch rollout that also
// write the world-frame records (rollout_kernel<GS, SAIL, MIXED, true>), handed to the launcher of ebcsim.hip
// (ebc_world_api.h).  The kernel is ebc_rollout.h's.
//
// The wave timeline and the withhold hook (ebc_trace.h) belong to ebcsim.hip, whose device globals they use: this unit is
// compiled without them in every build.
#undef EBC_WAVE_TRACE
#include <hip/hip_runtime.h>

#include "ebc_group_sizes.h"
#include "ebc_kernels.h"
#include "ebc_rollout.h"
#include "ebc_world_api.h"

namespace ebc_world_api {

using ebc_host::kDevHumanGs;
using ebc_host::with_group_size;

int rollout_kernel(int gs, bool sail, bool mixed, const void **kernel) {
  return with_group_size<kDevHumanGs>(gs, [&](auto g) -> int {
    constexpr int GS = decltype(g)::value;
    if (sail)
      *kernel = mixed ? (const void *)ebc::rollout_kernel<GS, true, true, true> : (const void *)ebc::rollout_kernel<GS, true, false, true>;
    else
      *kernel = mixed ? (const void *)ebc::rollout_kernel<GS, false, true, true> : (const void *)ebc::rollout_kernel<GS, false, false, true>;
    return EBC_OK;
  });
}

}  // namespace ebc_world_api
