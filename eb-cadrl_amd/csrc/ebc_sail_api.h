// ebc_sail_api.h — what ebcsim.hip (ebc_step_k with EBC_ROBOT_SAIL) needs of a network made by ebc_sail_create,
// defined in ebcsim_sail.hip: the packed weight image on the device, adult_num, and the launch of sail_kernel.
#pragma once

#include <hip/hip_runtime.h>

namespace ebc_sail_api {

struct View {
  const float *P;  // the packed image (ebc_sail_rule.h: pack), device memory owned by the network
  int N;           // adult_num
  int device;
};

// the view of an ebc_sail_create handle
View view(void *sail);

// one sail_kernel launch on `stream`: robot [E][9], ob [E][R][5], n_rows [E] or nullptr -> action [E][2]
int launch(const float *P, int N, hipStream_t stream, const double *robot, const double *ob, const long long *n_rows,
           double *action, float *feat_joint, int E, int R);

// device memory the network owns for ebc_sail_grad (ebcsim_sail_grad.hip), at least `bytes`, grown on demand and freed
// by ebc_sail_destroy
int grad_scratch(void *sail, size_t bytes, void **out);

}  // namespace ebc_sail_api
