// ebc_group_sizes.h — the one switch from a run-time ORCA group size to a compile-time one, shared by the units that
// instantiate kernels per group size (ebcsim.hip, which also holds the table kGroupSizes, and ebcsim_mix.hip).
#pragma once

#include <string>
#include <type_traits>

#include "ebc_host.h"

namespace ebc_host {

// Development builds (make dev) instantiate ONE group size per kind of kernel: EBC_DEV_GS for the kernels
// of the humans' ORCA, 21 for the robot's.  0 = every size of kGroupSizes.
#ifdef EBC_DEV_GS
constexpr int kDevHumanGs = EBC_DEV_GS, kDevRobotGs = 21;
#else
constexpr int kDevHumanGs = 0, kDevRobotGs = 0;
#endif

// Run-time group size -> compile-time one: calls f(std::integral_constant<int, GS>()) for GS == gs, a member of
// kGroupSizes.  The only place that lists the instantiated sizes besides the table.
template <int DEV_GS, typename F>
int with_group_size(int gs, F f) {
  if constexpr (DEV_GS != 0) {
    if (gs != DEV_GS) return fail(EBC_ERR_UNSUPPORTED, "development build: " + std::to_string(DEV_GS) + "-lane ORCA groups only");
    return f(std::integral_constant<int, DEV_GS>());
  } else {
    switch (gs) {
#define GS_(N) case N: return f(std::integral_constant<int, N>())
      GS_(2); GS_(3); GS_(4); GS_(5); GS_(6); GS_(7); GS_(8); GS_(9); GS_(10); GS_(12); GS_(16); GS_(21);
#undef GS_
      default: return f(std::integral_constant<int, 32>());
    }
  }
}

}  // namespace ebc_host
