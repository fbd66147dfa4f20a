// ebc_local_map_kernel.h — get_local_map_angular (simulator/env.py:468-628) for every env of a batch, on the device.
//
// One wave per env.  The env's polygons are those of its scene slot (DevState::grid_scene, the slot whose occupancy
// grid it runs: restarts rewrite it, so a map needs no change to any step kernel).  Polygons are taken four at a
// time: lane l builds table entry (polygon l / 16, vertex (l / 4) % 4, corner l % 4) — the vertex's sector and
// distance seen from the corner (ebc_local_map.h) — in LDS, then the 4 x 48 walks of those polygons (24 segment walks
// of phase 1, 24 constant fills of phase 2) are dealt out one per lane.  Sector minima go through LDS as a 64-bit
// unsigned atomicMin on the bit pattern, which is the float minimum for the non-negative distances: exact, and
// independent of the order of the updates.
#pragma once

#include "ebc_kernels.h"
#include "ebc_local_map.h"

namespace ebc {

struct LocalMapIO {
  LocalMapCfg c;
  const double *poly;  // [slots][S][4][2]
  const int *n_poly;   // [slots]
  int S;
  int next;            // 1: the map of the state after this step's robot action (ebc_step_with_map)
  int robot_policy;    // with `next`: EBC_ROBOT_LINEAR or EBC_ROBOT_EXTERNAL (robot_action [E][2])
  const double *robot_action;
  double *out;         // [E][dim]
};

// (j, k) of the six vertex pairs of a walk set, j < k
__device__ __forceinline__ void lm_pair(int w, int &j, int &k) {
  k = w < 1 ? 1 : (w < 3 ? 2 : 3);
  j = w - (k == 1 ? 0 : (k == 2 ? 1 : 3));
}

// Before the pool arrays are replaced on a running batch (ebc_set_scene_pool / ebc_generate_pool): the polygons of the
// slot env e runs move into the env's own slot e, like its occupancy grid (rehome_grid_kernel, which runs next and
// points the env at slot e).
__global__ __launch_bounds__(64) void rehome_poly_kernel(DevState s, double *poly, int *n_poly, int S) {
  const int e = blockIdx.x;
  const int src = s.grid_scene[e];
  if (src == e) return;
  for (int w = threadIdx.x; w < S * 8; w += blockDim.x) poly[(size_t)e * S * 8 + w] = poly[(size_t)src * S * 8 + w];
  if (threadIdx.x == 0) n_poly[e] = n_poly[src];
}

__global__ __launch_bounds__(EBC_WAVE) void local_map_kernel(EbcParams p, DevState s, LocalMapIO io) {
  __shared__ unsigned long long rdv[EBC_LM_MAX_DIM];
  __shared__ int sec[64];
  __shared__ double dist[64];
  __shared__ double vert[16][2];
  const int e = blockIdx.x, lane = threadIdx.x;
  const LocalMapCfg &c = io.c;
  double rb[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) rb[q] = s.robot[(size_t)e * 9 + q];
  if (io.next) {  // the robot's next state, as every role of the step works it out (robot_action / robot_advance)
    double a0, a1;
    robot_action(io.robot_policy, io.robot_action, (size_t)e, rb, a0, a1);
    robot_advance(p, rb, a0, a1);
  }
  const double px = rb[0], py = rb[1], radius = rb[4], theta = rb[8];
  double cs, sn;
  sincos_dd(theta, cs, sn);
  const unsigned long long init = (unsigned long long)__double_as_longlong(c.max_range);
  for (int k = lane; k < c.dim; k += EBC_WAVE) rdv[k] = init;
  const int slot = s.grid_scene[e];
  int n = io.n_poly[slot];
  n = n < io.S ? n : io.S;
  const double *poly = io.poly + (size_t)slot * io.S * 8;
  // this lane's table entry: vertex vj of polygon pl of the group, seen from corner cq
  const int pl = lane >> 4, vj = (lane >> 2) & 3, cq = lane & 3;
  double ex, ey;
  lm_corner(cq, px, py, radius, ex, ey);
  auto put = [&](int k, double d) { atomicMin(&rdv[k], (unsigned long long)__double_as_longlong(d)); };
  for (int p0 = 0; p0 < n; p0 += 4) {
    __syncthreads();  // the previous group's walks are done with the table (and rdv is initialised)
    if (p0 + pl < n) {
      const double vx = poly[(size_t)(p0 + pl) * 8 + 2 * vj], vy = poly[(size_t)(p0 + pl) * 8 + 2 * vj + 1];
      int sc;
      double d;
      lm_entry(c, vx, vy, ex, ey, cs, sn, sc, d);
      sec[lane] = sc;
      dist[lane] = d;
      if (cq == 0) {
        vert[lane >> 2][0] = vx;
        vert[lane >> 2][1] = vy;
      }
      if (0 <= sc && sc < c.dim) put(sc, d);
    }
    __syncthreads();
    for (int w = lane; w < 4 * 48; w += EBC_WAVE) {
      const int pw = w / 48, r = w - pw * 48;
      if (p0 + pw >= n) break;  // w grows with the lane's loop: the rest lie past the last polygon too
      const int base = pw * 16;
      int j, k;
      if (r < 24) {  // phase 1: corner q, the segment between vertices j < k (env.py:590-606)
        const int q = r / 6;
        lm_pair(r - q * 6, j, k);
        const LmWalk wk = lm_walk(c, sec[base + k * 4 + q], sec[base + j * 4 + q]);
        const int a = wk.from_new ? k : j, b = wk.from_new ? j : k;
        int i0, i1;
        lm_walk_range(c, wk, i0, i1);
        if (i0 < i1) {
          double qx, qy;
          lm_corner(q, px, py, radius, qx, qy);
          const double ax = vert[pw * 4 + a][0], ay = vert[pw * 4 + a][1];
          const double bx = vert[pw * 4 + b][0], by = vert[pw * 4 + b][1];
          for (int i = i0; i < i1; ++i) put(wk.start + i, lm_walk_point(i, wk.span, ax, ay, bx, by, qx, qy, cs, sn));
        }
      } else {  // phase 2: vertex v, corners j < k: the distance from corner k over the walk (env.py:607-621)
        const int v = (r - 24) / 6;
        lm_pair(r - 24 - v * 6, j, k);
        const LmWalk wk = lm_walk(c, sec[base + v * 4 + k], sec[base + v * 4 + j]);
        int i0, i1;
        lm_walk_range(c, wk, i0, i1);
        const double d = dist[base + v * 4 + k];
        for (int i = i0; i < i1; ++i) put(wk.start + i, d);
      }
    }
  }
  __syncthreads();
  double *out = io.out + (size_t)e * c.dim;
  for (int k = lane; k < c.dim; k += EBC_WAVE) {
    const double d = __longlong_as_double((long long)rdv[k]);
    out[k] = c.normalize ? d / c.max_range : d;
  }
}

}  // namespace ebc
