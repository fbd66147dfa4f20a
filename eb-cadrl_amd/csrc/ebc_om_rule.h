// ebc_om_rule.h — the arithmetic of an occupancy map (rl/policy/multi_human_rl.py:156-227), ONE definition for the
// kernel (hipcc, ebc_om.h) and for the host build the tests compare it with (g++, tests/native/om_host.cc).
//
// The reference turns every OTHER row o into the frame of row a (x axis along a's velocity) with arctan2 / cos / sin.
// Here the frame is algebraic:
//   sp = sqrt(vx^2 + vy^2);  (c, s) = (vx / sp, vy / sp);  sp == 0: (c, s) = (+1, 0) for vx = +0 and (-1, 0) for vx = -0
//                            (arctan2(+-0, +0) = +-0, arctan2(+-0, -0) = +-pi)
//   position of o:  (dx c + dy s, dy c - dx s)  with (dx, dy) = o - a
//   velocity of o:  (ovx c + ovy s, ovy c - ovx s)
//   cell:           ix = floor(x / cell_size + cell_num / 2), iy likewise; outside [0, cell_num) the occupant is dropped;
//                   k = cell_num * iy + ix
//   a cell:         channels 1: occupied 0 / 1;  2: the mean velocity of its occupants (vx, vy);  3: (1, mean vx, mean vy);
//                   an empty cell is 0.  The sums start at +0 and run over the occupants in row order in float64, are
//                   divided by the count, and are cast to float32 once.
// Every operation is rounded on its own (both builds compile with -ffp-contract=off); no libm beyond sqrt and floor.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EBC_OM_HD __host__ __device__ inline
#else
#define EBC_OM_HD inline
#endif

#define EBC_OM_MAX_ROWS 128
#define EBC_OM_MAX_ACTIONS 128
#define EBC_OM_MAX_WIDTH 192       // cell_num^2 * channels
#define EBC_OM_MAX_ROW_WIDTH 224   // T + W: what the two-layer blocks take as input

namespace ebc_om {

// the rows an env holds: n_valid clamped to [0, R]
EBC_OM_HD int clamp_rows(long long v, int R) { return v < 0 ? 0 : (v > R ? R : (int)v); }

EBC_OM_HD bool negative_bit(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u >> 63) != 0;
}

struct Frame {
  double c, s;
};

// the frame of a row that moves with (vx, vy)
EBC_OM_HD Frame frame(double vx, double vy) {
  const double xx = vx * vx, yy = vy * vy;
  const double sp = sqrt(xx + yy);
  Frame f;
  if (sp == 0.0) {
    f.c = negative_bit(vx) ? -1.0 : 1.0;
    f.s = 0.0;
  } else {
    f.c = vx / sp;
    f.s = vy / sp;
  }
  return f;
}

// the index of one axis, or -1 outside the grid (a NaN coordinate is outside)
EBC_OM_HD int axis_index(double coord, int cell_num, double cell_size) {
  const double q = coord / cell_size;
  const double i = floor(q + 0.5 * (double)cell_num);
  return (i >= 0.0 && i < (double)cell_num) ? (int)i : -1;
}

// the cell of the occupant at (ox, oy) in the map of the row at (ax, ay) with frame f, or -1
EBC_OM_HD int pair_cell(double ax, double ay, Frame f, double ox, double oy, int cell_num, double cell_size) {
  const double dx = ox - ax, dy = oy - ay;
  const double xc = dx * f.c, ys = dy * f.s, yc = dy * f.c, xs = dx * f.s;
  const int ix = axis_index(xc + ys, cell_num, cell_size), iy = axis_index(yc - xs, cell_num, cell_size);
  return (ix < 0 || iy < 0) ? -1 : cell_num * iy + ix;
}

// cell k of the map of row a, finished: `channels` floats.  px / py / vx / vy: the columns of the env's rows, `stride`
// doubles apart; rows [0, n) exist, and every one of them but a itself (by index: two rows at the same place still see
// each other) is an occupant.
EBC_OM_HD void finished_cell(const double *px, const double *py, const double *vx, const double *vy, int stride, int n, int a,
                             Frame f, int k, int cell_num, double cell_size, int channels, float *out) {
  const double ax = px[(size_t)a * stride], ay = py[(size_t)a * stride];
  int count = 0;
  double sx = 0.0, sy = 0.0;
  for (int o = 0; o < n; ++o) {
    if (o == a) continue;
    const size_t at = (size_t)o * stride;
    if (pair_cell(ax, ay, f, px[at], py[at], cell_num, cell_size) != k) continue;
    ++count;
    if (channels > 1) {
      const double ovx = vx[at], ovy = vy[at];
      const double xc = ovx * f.c, ys = ovy * f.s, yc = ovy * f.c, xs = ovx * f.s;
      sx = sx + (xc + ys);
      sy = sy + (yc - xs);
    }
  }
  if (channels == 1) {
    out[0] = count ? 1.0f : 0.0f;
    return;
  }
  float *v = out + (channels - 2);
  if (channels == 3) out[0] = count ? 1.0f : 0.0f;
  v[0] = count ? (float)(sx / (double)count) : 0.0f;
  v[1] = count ? (float)(sy / (double)count) : 0.0f;
}

}  // namespace ebc_om
