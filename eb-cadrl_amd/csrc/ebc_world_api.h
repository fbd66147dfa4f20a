// ebc_world_api.h — what ebcsim.hip sees of ebcsim_world.hip, the unit that holds ebc_step_k_world's instantiations of the
// one-launch rollout (rollout_kernel<GS, SAIL, MIXED, true>).  Their third argument is RolloutIOWorld<SAIL>
// (ebc_rollout.h): the argument of the default instantiation with the two record pointers behind it.  A unit of their own,
// as ebcsim_mix.hip is, so that the instantiations of plain ebc_step_k are compiled as they were.
#pragma once

namespace ebc_world_api {

// The kernel for `gs` lanes per human (a member of the instantiated sizes); the error is set when the build has none.
int rollout_kernel(int gs, bool sail, bool mixed, const void **kernel);

}  // namespace ebc_world_api
