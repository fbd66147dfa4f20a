// ebc_om.h — the occupancy maps of rl/policy/multi_human_rl.py:156-227 and the rows the value network sees with them
// (:62-69) as one kernel.  The arithmetic is ebc_om_rule.h.
//
// A workgroup per (env, share of the env's actions).  The env's rows that exist go into LDS once with their frames; a
// thread per (row, cell) walks the other rows in row order and leaves the finished cell in LDS (no atomics: the sum of a
// cell is one thread's, in row order, so no launch shape changes a bit of it); rows at or past the env's count are never
// read and get zero maps.  Every workgroup of an env computes the same maps (a few hundred pair tests at the sizes a
// decision has), the first one stores them as `om`.
//
// Then the workgroup streams its actions' wide rows: the env's A * R * (T + W) floats are ONE contiguous run, so the
// share [a0, a1) of it is written as a flat run too — scalar stores up to the first 16-byte boundary, float4 stores from
// there, scalar stores for what is left — whatever T + W is; each float comes from `rows` (column < T) or from the maps
// in LDS.  This phase is the only one that moves real memory.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_om_rule.h"

#define EBC_OM_THREADS 256

namespace ebc {

struct OmLaunch {
  const double *next_ob;     // [E][R][5]
  const long long *n_valid;  // [E] or nullptr = R
  const float *rows;         // [E][A][R][T] or nullptr
  float *om;                 // [E][R][W] or nullptr
  float *rows_wide;          // [E][A][R][T + W] or nullptr
  double cell_size;
  int cell_num, channels, A, R, T;
};

// LDS: six double columns of R rows (px, py, vx, vy, frame c, frame s), then the maps [R][W] float
__host__ __device__ inline size_t om_lds_bytes(int R, int W) { return (size_t)R * 6 * sizeof(double) + (size_t)R * W * sizeof(float); }

__global__ __launch_bounds__(EBC_OM_THREADS) void occupancy_rows_kernel(const OmLaunch a) {
  extern __shared__ double om_lds[];
  const int tid = threadIdx.x, R = a.R, cells = a.cell_num * a.cell_num, C = a.channels, W = cells * C;
  double *px = om_lds, *py = px + R, *vx = py + R, *vy = vx + R, *fc = vy + R, *fs = fc + R;
  float *maps = reinterpret_cast<float *>(fs + R);
  const size_t e = blockIdx.x;
  const int n = ebc_om::clamp_rows(a.n_valid ? a.n_valid[e] : (long long)R, R);
  for (int r = tid; r < n; r += EBC_OM_THREADS) {
    const double *o = a.next_ob + (e * R + r) * 5;
    const double x = o[0], y = o[1], u = o[2], v = o[3];
    const ebc_om::Frame f = ebc_om::frame(u, v);
    px[r] = x; py[r] = y; vx[r] = u; vy[r] = v; fc[r] = f.c; fs[r] = f.s;
  }
  __syncthreads();
  for (int i = tid; i < R * cells; i += EBC_OM_THREADS) {
    const int row = i / cells, k = i - row * cells;
    float *out = maps + (size_t)row * W + (size_t)k * C;
    if (row < n) {
      ebc_om::Frame f;
      f.c = fc[row];
      f.s = fs[row];
      ebc_om::finished_cell(px, py, vx, vy, 1, n, row, f, k, a.cell_num, a.cell_size, C, out);
    } else {
      for (int c = 0; c < C; ++c) out[c] = 0.0f;
    }
  }
  __syncthreads();
  if (a.om && blockIdx.y == 0) {
    float *om = a.om + e * R * W;
    for (int i = tid; i < R * W; i += EBC_OM_THREADS) om[i] = maps[i];
  }
  if (!a.rows_wide) return;

  const int T = a.T, TW = T + W, A = a.A;
  const int a0 = (int)((long long)A * blockIdx.y / gridDim.y), a1 = (int)((long long)A * (blockIdx.y + 1) / gridDim.y);
  const int g0 = a0 * R * TW, g1 = a1 * R * TW;  // this workgroup's run inside the env's A * R * TW floats (< 2^22)
  float *dst = a.rows_wide + e * A * R * TW;
  const float *src = a.rows + e * A * R * T;
  // float g of the env's run: row slot q = g / TW (action-major), column g % TW
  auto value = [&](int q, int col) -> float { return col < T ? src[(size_t)q * T + col] : maps[(q % R) * W + (col - T)]; };
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(dst + g0) >> 2) & 3)) & 3);
  if (head > g1 - g0) head = g1 - g0;
  if (tid < head) {
    const int g = g0 + tid;
    dst[g] = value(g / TW, g % TW);
  }
  const int v0 = g0 + head, nvec = (g1 - v0) >> 2;
  for (int j = tid; j < nvec; j += EBC_OM_THREADS) {
    const int g = v0 + 4 * j;
    int q = g / TW, col = g - q * TW;
    float x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = value(q, col);
      if (++col == TW) {
        col = 0;
        ++q;
      }
    }
    *reinterpret_cast<float4 *>(dst + g) = make_float4(x[0], x[1], x[2], x[3]);
  }
  const int t0 = v0 + 4 * nvec;
  if (tid < g1 - t0) {
    const int g = t0 + tid;
    dst[g] = value(g / TW, g % TW);
  }
}

}  // namespace ebc
