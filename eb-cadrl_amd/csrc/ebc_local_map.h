// ebc_local_map.h — get_local_map_angular (simulator/env.py:468-628) of one env, host and device from one source.
//
// The reference starts from `dim` sectors at max_range and takes sector minima of the distances between the four
// corners of the robot's box (px +- radius, py +- radius) and the obstacle polygons, in the robot's heading frame
// (calculate_angular_map_distances, :468-568, called from :570-628 in two loops):
//   phase 1 (:590-606): per (polygon, corner), the polygon's vertices one after the other; every new vertex is
//     stored at its sector and, for every earlier vertex, the sectors between the two are filled by walking along
//     the segment in steps of 1 / span (one interpolated point per covered sector, measured from that corner);
//   phase 2 (:607-621): per (polygon, vertex), the four corners one after the other; the segment's two ends are the
//     same vertex, so every point of a walk is the vertex itself, measured from the NEWER corner: a walk fills its
//     sectors with one value of the (vertex, corner) table.
// Every update is rdv[k] = min(rdv[k], d) with d >= 0, so the order of updates does not matter.  What this file keeps
// of the reference, operation for operation (ebcsim/local_map.py restates it in Python):
//   - the rotated offset rx = dx cos + dy sin, ry = dy cos - dx sin, unfused (-ffp-contract=off), and its sector
//     int((atan2(ry, rx) - angle_min) / res), truncated toward zero; a sector outside [0, dim) is never stored but
//     still takes part in walks (atan2(+0, x < 0) = +pi gives sector dim with angles +-pi);
//   - the wrap test |sector - old| > pi / res (an int against a double), and the spans it implies; a walk covers
//     [start, start + span) clipped to [0, dim): the part of a "wrapped" walk beyond dim is dropped (:556-566 only
//     store (start + i) % dim while start + i < dim);
//   - np.linalg.norm of the offset as ebc::norm2 computes it (the second product fused, ebc_device.h);
//   - cos / sin of theta from sincos_dd (ebc_scene_gen.h): correctly rounded in all but ~2^-12 of the cases, the
//     same bits on the host and on the device.  atan2 is the platform's (libm / ocml); it only picks sectors.
// The kernel (ebc_local_map_kernel.h) and tests/native/local_map_host.cc both call the functions below.
#pragma once

#include "ebc_scene_gen.h"

#define EBC_LM_MAX_DIM 128

namespace ebc {

struct LocalMapCfg {
  int dim;
  int normalize;
  double max_range, angle_min, angle_max;
  double res;          // (angle_max - angle_min) / dim, env.py:588
  double pi_over_res;  // np.pi / res: the wrap test, env.py:533
};

EBC_HD LocalMapCfg local_map_cfg(int dim, double max_range, double angle_min, double angle_max, int normalize) {
  LocalMapCfg c;
  c.dim = dim;
  c.normalize = normalize;
  c.max_range = max_range;
  c.angle_min = angle_min;
  c.angle_max = angle_max;
  c.res = (angle_max - angle_min) / (double)dim;
  c.pi_over_res = 3.141592653589793 / c.res;
  return c;
}

// np.linalg.norm((x, y)): the two-element dot with the second product fused (same form as ebc::norm2)
EBC_HD double lm_norm(double x, double y) { return sqrt(fma(y, y, x * x)); }

// polar() of env.py:490-497: (x, y) relative to corner (ex, ey), rotated into the heading frame
EBC_HD void lm_rotate(double x, double y, double ex, double ey, double cs, double sn, double &rx, double &ry) {
  rx = (x - ex) * cs + (y - ey) * sn;
  ry = (y - ey) * cs - (x - ex) * sn;
}

// One (vertex, corner) entry of the table: the vertex's sector and distance seen from the corner (env.py:498-505)
EBC_HD void lm_entry(const LocalMapCfg &c, double vx, double vy, double ex, double ey, double cs, double sn,
                     int &sector, double &dist) {
  double rx, ry;
  lm_rotate(vx, vy, ex, ey, cs, sn, rx, ry);
  sector = (int)((atan2(ry, rx) - c.angle_min) / c.res);
  dist = lm_norm(rx, ry);
}

// The walk between an earlier point (sector `old`) and a new one (`sector`), env.py:530-566: its first sector,
// its span, and whether it runs from the new point to the old one.
struct LmWalk {
  int start, span;
  bool from_new;
};
EBC_HD LmWalk lm_walk(const LocalMapCfg &c, int sector, int old) {
  const int diff = sector > old ? sector - old : old - sector;
  const bool wrapped = (double)diff > c.pi_over_res;
  LmWalk w;
  if (wrapped)
    w.span = sector > old ? c.dim - sector + old : c.dim - old + sector;
  else
    w.span = diff;
  w.from_new = (sector < old && !wrapped) || (sector > old && wrapped);
  w.start = w.from_new ? sector : old;
  return w;
}
// The steps i of a walk whose sector start + i lies in [0, dim): [i0, i1)
EBC_HD void lm_walk_range(const LocalMapCfg &c, const LmWalk &w, int &i0, int &i1) {
  i0 = w.start < 0 ? -w.start : 0;
  i1 = c.dim - w.start < w.span ? c.dim - w.start : w.span;
  if (i1 < i0) i1 = i0;
}
// Step i of a phase-1 walk from (ax, ay) to (bx, by), measured from corner (ex, ey) (env.py:559-565)
EBC_HD double lm_walk_point(int i, int span, double ax, double ay, double bx, double by, double ex, double ey,
                            double cs, double sn) {
  const double t = (double)i / (double)span;
  double rx, ry;
  lm_rotate(ax + t * (bx - ax), ay + t * (by - ay), ex, ey, cs, sn, rx, ry);
  return lm_norm(rx, ry);
}

// Corner q of the robot's box (env.py:580-586): (-,-), (+,-), (-,+), (+,+)
EBC_HD void lm_corner(int q, double px, double py, double radius, double &ex, double &ey) {
  ex = (q & 1) ? px + radius : px - radius;
  ey = (q & 2) ? py + radius : py - radius;
}

// The plain per-env loop (host build, tests): poly [n_poly][4][2], out [dim]
EBC_HD void local_map_env(const LocalMapCfg &c, const double *poly, int n_poly, double px, double py, double radius,
                          double theta, double *out) {
  double cs, sn;
  sincos_dd(theta, cs, sn);
  for (int k = 0; k < c.dim; ++k) out[k] = c.max_range;
  auto put = [&](int k, double d) {
    if (d < out[k]) out[k] = d;
  };
  for (int p = 0; p < n_poly; ++p) {
    const double *v = poly + (size_t)p * 8;
    int sec[4][4];  // [vertex][corner]
    double dist[4][4];
    double ex[4], ey[4];
    for (int q = 0; q < 4; ++q) lm_corner(q, px, py, radius, ex[q], ey[q]);
    for (int j = 0; j < 4; ++j)
      for (int q = 0; q < 4; ++q) {
        lm_entry(c, v[2 * j], v[2 * j + 1], ex[q], ey[q], cs, sn, sec[j][q], dist[j][q]);
        if (0 <= sec[j][q] && sec[j][q] < c.dim) put(sec[j][q], dist[j][q]);
      }
    // phase 1: per corner q, vertex pairs j < k
    for (int q = 0; q < 4; ++q)
      for (int k = 1; k < 4; ++k)
        for (int j = 0; j < k; ++j) {
          const LmWalk w = lm_walk(c, sec[k][q], sec[j][q]);
          const int a = w.from_new ? k : j, b = w.from_new ? j : k;
          int i0, i1;
          lm_walk_range(c, w, i0, i1);
          for (int i = i0; i < i1; ++i)
            put(w.start + i, lm_walk_point(i, w.span, v[2 * a], v[2 * a + 1], v[2 * b], v[2 * b + 1], ex[q], ey[q], cs, sn));
        }
    // phase 2: per vertex j, corner pairs q0 < q1, the value of (j, q1)
    for (int j = 0; j < 4; ++j)
      for (int q1 = 1; q1 < 4; ++q1)
        for (int q0 = 0; q0 < q1; ++q0) {
          const LmWalk w = lm_walk(c, sec[j][q1], sec[j][q0]);
          int i0, i1;
          lm_walk_range(c, w, i0, i1);
          for (int i = i0; i < i1; ++i) put(w.start + i, dist[j][q1]);
        }
  }
  if (c.normalize)
    for (int k = 0; k < c.dim; ++k) out[k] = out[k] / c.max_range;
}

}  // namespace ebc
