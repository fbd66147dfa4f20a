// ebcsim_orca_wide.hip — the robot's ORCA solve on observations of 33 .. 128 rows: orca_robot_wide_kernel
// (ebc_orca_wide.h), handed to launch_robot_orca of ebcsim.hip (ebc_orca_wide_api.h).
//
// The wave timeline and the withhold hook (ebc_trace.h) belong to ebcsim.hip, whose device globals they use: this unit is
// compiled without them in every build.
#undef EBC_WAVE_TRACE
#include <hip/hip_runtime.h>

#include <cstddef>

#include "ebc_orca_wide.h"
#include "ebc_orca_wide_api.h"

static_assert(EBC_OW_LANES * EBC_OW_SLOTS == EBC_OW_ROWS && EBC_OW_ROWS % 4 == 0, "a lane's rows cover the handle's row limit");
static_assert(sizeof(ebc::OrcaWideLds) % 16 == 0 && offsetof(ebc::OrcaWideLds, dist) % 16 == 0 &&
                  offsetof(ebc::OrcaWideLds, pv) % 16 == 0,
              "the float4 reads of the LDS arrays are aligned");

namespace ebc_orca_wide_api {

void robot_kernel(const void **kernel, int *envs_per_block) {
  *kernel = (const void *)ebc::orca_robot_wide_kernel;
  *envs_per_block = EBC_OW_ENVS;
}

}  // namespace ebc_orca_wide_api
