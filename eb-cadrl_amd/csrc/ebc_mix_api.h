// ebc_mix_api.h — what ebcsim.hip sees of ebcsim_mix.hip, the unit that holds EBC_HUMAN_BY_TYPE's instantiations of the
// fused step (orca_step_kernel<GS, T, true>) and of the one-launch rollout (rollout_kernel<GS, SAIL, true>).  They take
// the arguments of the default instantiations, so the launchers of ebcsim.hip serve both: this unit only hands out the
// kernels.  A unit of their own, compiled beside the others, so that the default instantiations are compiled as they
// were and the build does not wait twice as long for ebcsim.hip.
#pragma once

namespace ebc_mix_api {

// The kernel for `gs` lanes per human (a member of the instantiated sizes); the error is set when the build has none.
int step_kernel(int gs, int T, const void **kernel);       // T = 13 or 17 floats per rotated row
int rollout_kernel(int gs, bool sail, const void **kernel);

}  // namespace ebc_mix_api
