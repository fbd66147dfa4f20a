// ebc_om_state.h — the state OM-SARL stores for training (rl/policy/multi_human_rl.py:128-149: transform(state) =
// [rotate(state) | build_occupancy_maps(state.agent_states)]) straight from the env's device state, as one kernel:
// ebc_observe_wide, and the extra enqueue per step of ebc_step_k_om; and the state OM-LSTM stores in RL, the same with the
// rows sorted by decreasing distance BEFORE the maps are built: ebc_observe_wide_sorted (below).  No arithmetic of its
// own: the rows are obs_row / rot_frame / rotate_row of the shared step rules, the maps are ebc_om_rule.h.
//
// A workgroup per env.  Phase 1, a thread per row slot: the row of the current state (what ebc_observe gives as `ob`)
// goes into LDS as double columns px, py, vx, vy with its map frame c, s — only the rows that exist, as
// occupancy_rows_kernel loads them — and its rotated floats (ebc_observe's obs_rotated: zeros for a slot without a row)
// go into LDS beside them.  Phase 2, a thread per (row, cell): walks the other rows in row order and leaves the finished
// cell in LDS; no atomics, so no launch shape changes a bit of a sum.  Phase 3: the env's R * (T + W) floats are ONE
// contiguous run and leave as one — scalar stores up to the first 16-byte boundary, float4 stores from there, scalar
// stores for what is left — whatever T + W is.
//
// LDS at the limits (R = 128, W = 192, T = 17): 6 KB of columns + 96 KB of maps + 8.5 KB of rotated rows = 110.5 KB of a
// workgroup's 160 KB.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_kernels.h"
#include "ebc_om_rule.h"

#define EBC_OMS_THREADS 256

namespace ebc {

struct OmStateSpec {
  double cell_size;
  int cell_num, channels;
};

// six double columns of R rows, the maps [R][W] float, the rotated rows [R][T] float
__host__ __device__ inline size_t om_state_lds_bytes(int R, int W, int T) {
  return (size_t)R * 6 * sizeof(double) + (size_t)R * (W + T) * sizeof(float);
}

// Phase 2 and 3 of a wide-state kernel, after its phase 1 has filled the columns, the frames and the rotated rows of the
// env's row slots (and the workgroup has met): the finished cells of rows [0, n) in LDS, zero maps behind them, then the
// env's R * (T + W) floats to dst as one run.
template <int T>
__device__ __forceinline__ void om_state_maps_and_store(const double *px, const double *py, const double *vx, const double *vy,
                                                        const double *fc, const double *fs, float *maps, const float *rot, int R,
                                                        int n, const OmStateSpec &spec, float *dst, int tid) {
  const int cells = spec.cell_num * spec.cell_num, C = spec.channels, W = cells * C;
  for (int i = tid; i < R * cells; i += EBC_OMS_THREADS) {
    const int row = i / cells, k = i - row * cells;
    float *out = maps + (size_t)row * W + (size_t)k * C;
    if (row < n) {
      ebc_om::Frame f;
      f.c = fc[row];
      f.s = fs[row];
      ebc_om::finished_cell(px, py, vx, vy, 1, n, row, f, k, spec.cell_num, spec.cell_size, C, out);
    } else {
      for (int c = 0; c < C; ++c) out[c] = 0.0f;
    }
  }
  __syncthreads();

  const int TW = T + W, total = R * TW;  // <= 128 * 224
  auto value = [&](int q, int col) -> float { return col < T ? rot[q * T + col] : maps[q * W + (col - T)]; };
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3);
  if (head > total) head = total;
  if (tid < head) dst[tid] = value(tid / TW, tid % TW);
  const int nvec = (total - head) >> 2;
  for (int j = tid; j < nvec; j += EBC_OMS_THREADS) {
    const int g = head + 4 * j;
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
  const int t0 = head + 4 * nvec;
  if (tid < total - t0) {
    const int g = t0 + tid;
    dst[g] = value(g / TW, g % TW);
  }
}

template <int T>
__global__ __launch_bounds__(EBC_OMS_THREADS) void observe_wide_kernel(EbcParams p, DevState s, OmStateSpec spec, float *state_wide,
                                                                        long long *n_rows) {
  extern __shared__ double oms_lds[];
  const int tid = threadIdx.x, R = s.N + s.S, cells = spec.cell_num * spec.cell_num, C = spec.channels, W = cells * C;
  double *px = oms_lds, *py = px + R, *vx = py + R, *vy = vx + R, *fc = vy + R, *fs = fc + R;
  float *maps = reinterpret_cast<float *>(fs + R);
  float *rot = maps + (size_t)R * W;
  const size_t e = blockIdx.x;
  const int nh = s.n_humans[e];
  const int ns = s.S ? s.n_static[e] : 0;
  const int n = ebc_om::clamp_rows((long long)nh + ns, R);  // row_counts_kernel's count; a handle holds nh <= N, ns <= S
  if (n_rows && tid == 0) n_rows[e] = (long long)nh + ns;
  const EnvRows<uint8_t> rows = env_rows(s, e);
  for (int r = tid; r < R; r += EBC_OMS_THREADS) {
    const ObsRow row = obs_row(rows, r, nh, ns);
    if (r < n) {
      const ebc_om::Frame f = ebc_om::frame(row.vx, row.vy);
      px[r] = row.px; py[r] = row.py; vx[r] = row.vx; vy[r] = row.vy; fc[r] = f.c; fs[r] = f.s;
    }
    float out[T];
    RotFrame f = {};  // a row that does not exist needs no frame
    if (row.valid) f = rot_frame(s.robot + e * 9, p.rotate_unicycle);
    rotated_row_or_zeros<T>(f, row, out);
#pragma unroll
    for (int c = 0; c < T; ++c) rot[r * T + c] = out[c];
  }
  __syncthreads();
  om_state_maps_and_store<T>(px, py, vx, vy, fc, fs, maps, rot, R, n, spec, state_wide + e * (size_t)R * (T + W), tid);
}

// ebc_observe_wide_sorted — the state OM-LSTM stores in RL (rl/policy/lstm_rl.py:117-123 sorts state.agent_states by
// decreasing distance to the robot, THEN transform(state) builds the maps from the sorted list): observe_wide_kernel with
// the env's existing rows put in that order before a map is built, so a cell's sums walk its occupants in sorted order.
// Phase 1 keeps the row, its map frame and its rotated floats in the thread's registers (a thread per row slot: R <= 128
// < EBC_OMS_THREADS) and leaves only the sort key in LDS: k = -da (the rotated row's own float32 column 11), +inf for a
// NaN da.  rank(r) = #{j < n : k_j < k_r, or k_j == k_r and j < r} is lstm_train.sort_rows_by_distance's stable order,
// counted by the row's own thread — no atomics, nothing a launch shape could change.  The thread then writes its columns
// and rotated floats at slot rank(r); slots >= n stay where they are.  Phases 2 and 3 are observe_wide_kernel's.
// LDS: om_state_lds_bytes plus R keys of 4 bytes.
#define EBC_OMS_KEY_COLUMN 11

__host__ __device__ inline size_t om_state_sorted_lds_bytes(int R, int W, int T) { return om_state_lds_bytes(R, W, T) + (size_t)R * sizeof(int); }

template <int T>
__global__ __launch_bounds__(EBC_OMS_THREADS) void observe_wide_sorted_kernel(EbcParams p, DevState s, OmStateSpec spec,
                                                                               float *state_wide, long long *n_rows) {
  extern __shared__ double oms_lds[];
  const int tid = threadIdx.x, R = s.N + s.S, W = spec.cell_num * spec.cell_num * spec.channels;
  double *px = oms_lds, *py = px + R, *vx = py + R, *vy = vx + R, *fc = vy + R, *fs = fc + R;
  float *maps = reinterpret_cast<float *>(fs + R);
  float *rot = maps + (size_t)R * W;
  float *key = rot + (size_t)R * T;
  const size_t e = blockIdx.x;
  const int nh = s.n_humans[e];
  const int ns = s.S ? s.n_static[e] : 0;
  const int n = ebc_om::clamp_rows((long long)nh + ns, R);
  if (n_rows && tid == 0) n_rows[e] = (long long)nh + ns;
  const int r = tid;
  ObsRow row = {0, 0, 0, 0, 0, 0, false};
  float out[T];
  if (r < R) {
    row = obs_row(env_rows(s, e), r, nh, ns);
    RotFrame f = {};  // a row that does not exist needs no frame
    if (row.valid) f = rot_frame(s.robot + e * 9, p.rotate_unicycle);
    rotated_row_or_zeros<T>(f, row, out);
    if (r < n) key[r] = out[EBC_OMS_KEY_COLUMN] != out[EBC_OMS_KEY_COLUMN] ? INFINITY : -out[EBC_OMS_KEY_COLUMN];
  }
  __syncthreads();
  if (r < R) {
    int slot = r;
    if (r < n) {
      const float k = key[r];
      slot = 0;
      for (int j = 0; j < n; ++j) {
        const float kj = key[j];
        slot += (kj < k || (kj == k && j < r)) ? 1 : 0;
      }
      const ebc_om::Frame f = ebc_om::frame(row.vx, row.vy);
      px[slot] = row.px; py[slot] = row.py; vx[slot] = row.vx; vy[slot] = row.vy; fc[slot] = f.c; fs[slot] = f.s;
    }
#pragma unroll
    for (int c = 0; c < T; ++c) rot[slot * T + c] = out[c];
  }
  __syncthreads();
  om_state_maps_and_store<T>(px, py, vx, vy, fc, fs, maps, rot, R, n, spec, state_wide + e * (size_t)R * (T + W), tid);
}

}  // namespace ebc
