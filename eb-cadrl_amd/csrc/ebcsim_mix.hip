// ebcsim_mix.hip — EBC_HUMAN_BY_TYPE (ebc_set_human_policies): the mixed instantiations of the fused step and of the
// one-launch rollout, handed to the launchers of ebcsim.hip (ebc_mix_api.h).  The kernels are ebc_kernels.h's and
// ebc_rollout.h's.
//
// The wave timeline and the withhold hook (ebc_trace.h) belong to ebcsim.hip, whose device globals they use: this unit is
// compiled without them in every build.
#undef EBC_WAVE_TRACE
#include <hip/hip_runtime.h>

#include "ebc_group_sizes.h"
#include "ebc_kernels.h"
#include "ebc_mix_api.h"
#include "ebc_rollout.h"

namespace ebc_mix_api {

using ebc_host::kDevHumanGs;
using ebc_host::with_group_size;

int step_kernel(int gs, int T, const void **kernel) {
  return with_group_size<kDevHumanGs>(gs, [&](auto g) -> int {
    constexpr int GS = decltype(g)::value;
    *kernel = T == 17 ? (const void *)ebc::orca_step_kernel<GS, 17, true> : (const void *)ebc::orca_step_kernel<GS, 13, true>;
    return EBC_OK;
  });
}

int rollout_kernel(int gs, bool sail, const void **kernel) {
  return with_group_size<kDevHumanGs>(gs, [&](auto g) -> int {
    constexpr int GS = decltype(g)::value;
    *kernel = sail ? (const void *)ebc::rollout_kernel<GS, true, true> : (const void *)ebc::rollout_kernel<GS, false, true>;
    return EBC_OK;
  });
}

}  // namespace ebc_mix_api
