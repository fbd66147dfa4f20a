// ebc_step_rules.h — the rules of one env.step that more than one kernel applies, each defined once.
//
// Every function takes values or plain pointers, so a caller feeds it from global memory (the service kernels of
// ebc_kernels.h) or from LDS (rollout_kernel, ebc_rollout.h) and the arithmetic is the same operation for operation.
// The per-step kernels (step_kernel, orca_step_kernel) keep their own copies of some of these rules: their instruction
// sequence is the measured headline, and a call in place of the copy moves it.  Each such copy
// carries a comment that names the definition here.
#pragma once

#include "ebc_device.h"

namespace ebc {

// Scenes an env restarts from under EBC_FLAG_AUTO_RESET, in the same SoA layout as the state.
// Slots [0, E) are the envs' own ebc_reset scenes; slots [E, E + P) a host-generated pool installed
// by ebc_set_scene_pool.  cursor[e] is the slot env e restarts from next: e itself without a pool
// (stride 0), else it walks E + (e mod P), + stride, ... (mod P) from episode to episode without
// leaving the device.  Occupancy grids are never copied: an env points at the grid of the slot it
// is running (grid_scene[e]).
struct ScenePool {
  int P, stride;  // custom scenes (0 = none) and the cursor step
  int *cursor;  // [E]
  int *n_humans;
  double *px, *py, *vx, *vy, *gx, *gy, *radius, *v_pref;
  uint8_t *type;
  int *n_static;
  double *spx, *spy, *sradius;
  uint64_t *grid;  // nullptr: free maps
  double *robot;
  float2 *pref;    // [slots][N] ORCA preferred velocity of the scene's humans (float tile, orca.py:136-140)
};

// The velocity the robot sweeps through the step with, from its action (collisions.py:29-57): what closest_dist takes.
__device__ __forceinline__ void swept_robot_velocity(int kinematics, double a0, double a1, double theta, double &rvx,
                                                     double &rvy) {
  if (kinematics == EBC_HOLONOMIC) {
    rvx = a0;
    rvy = a1;
  } else {
    rvx = a0 * cos(a1 + theta);
    rvy = a0 * sin(a1 + theta);
  }
}

// compute_collisions (env.py:303-338): the humans of an env in index order, per type the minimum distance of those
// before the type's first hit, and whether there was one.  A NaN distance neither hits nor lowers a minimum.
struct TypeWalk {
  double dmin[3] = {INFINITY, INFINITY, INFINITY};
  int coll[3] = {0, 0, 0};
  __device__ __forceinline__ void visit(double d, int type) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (type == q && !coll[q]) {
        if (d < 0) coll[q] = 1;
        else if (d < dmin[q]) dmin[q] = d;
      }
    }
  }
};

// What a step returns for one env, at index o of the outputs the caller asked for (IO: StepIO or RolloutIO).
template <typename IO>
__device__ __forceinline__ void store_outcome(const IO &io, size_t o, const RewardOut &ro, const double (&dmin)[3], double a0,
                                              double a1) {
  if (io.reward) io.reward[o] = ro.reward;
  if (io.done) io.done[o] = (uint8_t)ro.done;
  if (io.info) io.info[o] = (uint8_t)ro.info;
  if (io.dmin) {
    io.dmin[3 * o] = dmin[0];
    io.dmin[3 * o + 1] = dmin[1];
    io.dmin[3 * o + 2] = dmin[2];
  }
  if (io.dist_to_goal) io.dist_to_goal[o] = ro.dist_to_goal;
  if (io.robot_action_out) {
    io.robot_action_out[2 * o] = a0;
    io.robot_action_out[2 * o + 1] = a1;
  }
}

// Row r of an env's observation in the world frame (env.py:381-382, :457-458): the humans, then the static obstacles as
// pedestrians with zero velocity and type EBC_ADULT_STATIC, then rows that do not exist (zeros, not valid).
struct ObsRow {
  double px, py, vx, vy, radius;
  int type;
  bool valid;
};
// The arrays a row is read from, in global memory or in LDS: per human field and per static field.  obs_row takes those
// of ONE env: at(first human, first static row) of the whole batch's.
template <typename TypeT>
struct EnvRows {
  const double *px, *py, *vx, *vy, *radius;
  const TypeT *type;
  const double *spx, *spy, *sradius;
  __device__ __forceinline__ EnvRows at(size_t k, size_t q) const {
    return {px + k, py + k, vx + k, vy + k, radius + k, type + k, spx + q, spy + q, sradius + q};
  }
};
template <typename TypeT>
__device__ __forceinline__ ObsRow obs_row(const EnvRows<TypeT> &a, int r, int n, int ns) {
  ObsRow o = {0, 0, 0, 0, 0, 0, false};
  if (r < n) {
    o = ObsRow{a.px[r], a.py[r], a.vx[r], a.vy[r], a.radius[r], (int)a.type[r], true};
  } else if (r - n < ns) {
    const int q = r - n;
    o = ObsRow{a.spx[q], a.spy[q], 0.0, 0.0, a.sradius[q], EBC_ADULT_STATIC, true};
  }
  return o;
}
// The row in the robot's frame f (rotate_row), or T zeros for a row that does not exist
template <int T>
__device__ __forceinline__ void rotated_row_or_zeros(const RotFrame &f, const ObsRow &row, float *out) {
  if (row.valid) {
    rotate_row<T>(f, row.px, row.py, row.vx, row.vy, row.radius, row.type, out);
  } else {
#pragma unroll
    for (int c = 0; c < T; ++c) out[c] = 0.0f;
  }
}

// `cnt` floats of an LDS row buffer -> dst in flat order, by THREADS threads: 16-byte stores between the first and the
// last 16-byte boundary of the destination, single floats before and behind.  The 4 T bytes of a row are not a multiple
// of 16: writing row by row costs T dword stores per lane and splits every 128-B line.  (Phase C of lookahead_kernel
// keeps its own copy of this function and of rotated_row_or_zeros: its sweep measured slower with the calls.)
template <int THREADS>
__device__ __forceinline__ void flush_rows(const float *buf, float *dst, int cnt, int tid) {
  int head = (int)(((16 - ((size_t)dst & 15)) & 15) >> 2);
  head = head < cnt ? head : cnt;
  if (tid < head) dst[tid] = buf[tid];
  const int body4 = (cnt - head) / 4;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  for (int v = tid; v < body4; v += THREADS) {
    const int f = head + 4 * v;
    const f32x4 w = {buf[f], buf[f + 1], buf[f + 2], buf[f + 3]};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4 *>(dst + f));  // nothing on the device reads the rows again
  }
  const int tail0 = head + 4 * body4;
  if (tid < cnt - tail0) dst[tail0 + tid] = buf[tail0 + tid];
}

// The slot an env restarts from after `cur`, with a custom pool installed (P.P > 0): the walk E + (e mod P), + stride, ...
__device__ __forceinline__ int pool_next_cursor(const ScenePool &P, int E, int cur) {
  const int nxt = cur - E + P.stride;
  return E + (nxt >= P.P ? nxt % P.P : nxt);
}

// What human slot i of an env takes when the env restarts from pool slot `cur`: the scene's values where the scene has
// such a human, zeros where it has not, and the two records of the float tile (orca.py:110-140) with the preferred
// velocity that pool_pref_kernel stored.
struct RestartHuman {
  double px, py, vx, vy, gx, gy, radius, v_pref;
  int type;
  float4 tile0, tile1;
};
__device__ __forceinline__ RestartHuman restart_human(const EbcParams &p, const ScenePool &P, int N, int cur, int i) {
  RestartHuman h = {0, 0, 0, 0, 0, 0, 0, 0, 0, make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
  if (i < P.n_humans[cur]) {
    const size_t src = (size_t)cur * N + i;
    h.px = P.px[src]; h.py = P.py[src]; h.vx = P.vx[src]; h.vy = P.vy[src];
    h.gx = P.gx[src]; h.gy = P.gy[src]; h.radius = P.radius[src]; h.v_pref = P.v_pref[src];
    h.type = (int)P.type[src];
    const float2 rp = P.pref[src];
    h.tile0 = make_float4((float)h.px, (float)h.py, (float)h.vx, (float)h.vy);
    h.tile1 = make_float4((float)(h.radius + 0.01 + p.orca_safety_space), (float)h.v_pref, rp.x, rp.y);
  }
  return h;
}

}  // namespace ebc
