// ebc_orca_wide_api.h — what ebcsim.hip sees of ebcsim_orca_wide.hip, the unit that holds the robot's ORCA solve for
// observations of 33 .. 128 rows (orca_robot_wide_kernel, ebc_orca_wide.h).  The kernel takes the arguments of
// orca_robot_kernel, so launch_robot_orca of ebcsim.hip serves both: this unit only hands out the kernel and its grid.
// A unit of its own, as ebcsim_mix.hip and ebcsim_world.hip are, so that the kernels of ebcsim.hip are compiled as they
// were.
#pragma once

namespace ebc_orca_wide_api {

// The kernel (arguments: EbcParams, DevState, double safety_space, double *act, RobotSim) and the envs one workgroup of
// EBC_WAVE threads serves.
void robot_kernel(const void **kernel, int *envs_per_block);

}  // namespace ebc_orca_wide_api
