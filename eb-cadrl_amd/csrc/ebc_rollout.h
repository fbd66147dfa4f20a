// ebc_rollout.h — ebc_step_k with EBC_FLAG_ONE_LAUNCH: K env.step calls of every env in ONE kernel launch.
//
// Scenes are independent, so K fused steps need no grid barrier and no hand-off between workgroups: one workgroup
// (EBC_RO_THREADS threads) owns `epg` consecutive envs for all K steps.  Their state is read once, lives in LDS for
// the whole launch and is written back once; per step only the requested outputs, robot_action[k], the window of the
// occupancy grid and — when an env ends under auto-reset — its restart scene cross the memory system.  The phases of
// a step are separated by two workgroup barriers; there are no mailboxes and no polling, hence no give-up path.
//
//   P1   (pre-step state)
//        all threads   state_rotated[k] rows -> LDS row buffer (they leave as 16-byte stores after the barrier)
//        all threads   ebc_step_k_world only (rollout_kernel<GS, SAIL, MIXED, true>): the robot array and the world-frame
//                      rows of the workgroup's envs, from LDS straight to the caller's [k] slices (world_store)
//        all waves     EBC_ROBOT_SAIL only (rollout_kernel<GS, true>): the attached network decides for the envs of the
//                      workgroup, a chunk of envs at a time through one LDS area (sail_group, ebc_sail.h), from the
//                      LDS state; the action goes to act[] and a barrier ends it
//        last wave     the robot side of the step, which needs nothing from the humans' ORCA: n_rows[k]; the robot's
//                      action (EBC_ROBOT_LINEAR / _EXTERNAL: a lane per env; EBC_ROBOT_ORCA: a 32-lane ORCA group per
//                      env over the N + S observation rows, with the persistent simulator when it is enabled); swept
//                      robot-human distances, a lane per human; then a lane per env: ordered per-type reduce, grid
//                      window, reward / done / info, the robot's next state and its frame
//        every wave    the humans' ORCA velocities, GS lanes per human, from the LDS tile (the last wave takes a
//                      share only when the robot is not on ORCA)
//   P3a  a thread per human: move, first arrival, next tile record, its obs_rotated[k] row; static and padding rows
//   P3b  (only in a workgroup where an env ended under auto-reset, behind a third barrier) the restart scene
//
// What is shared.  The leaf arithmetic (orca_group, closest_dist, grid_collision, reward_compute, rot_frame, ...) and
// the step rules around it are called, not copied; the rules take values and plain pointers, and here they get the LDS
// state.  From ebc_step_rules.h: swept_robot_velocity, TypeWalk (the ordered per-type walk), store_outcome, obs_row +
// rotated_row_or_zeros (every row of state_rotated and obs_rotated, and the rows the SAIL network reads), flush_rows,
// restart_human and pool_next_cursor.  From ebc_kernels.h: robot_action, orca_robot_solve (the robot's ORCA with the
// persistent-simulator rule, as orca_robot_kernel and dagger_label_kernel call it) and orca_tile_load +
// orca_wave_compute (a human's ORCA, as the ORCA role of the per-step launch calls it).  What stays written out here
// is what only this form does: the moved human's commit on LDS arrays (P3a) and the copies between global memory and
// LDS.  The per-step kernels keep copies of some rules (the comments there name them): their emitted code is the
// measured headline and a call moves it.  So a change to one of those rules is made in ebc_step_rules.h and at the
// copies that name it, and tests/test_step_k_one_launch_gpu.py compares the two forms byte for byte.
//
// The arithmetic is that of the per-step form, operation for operation (ebc_device.h, ebc_orca_group.h; the unit is
// built with -ffp-contract=off): what the per-step kernels compute across several waves and launches is computed
// here from the same inputs in the same order, so every output and the state left behind are bit-identical
// (tests/test_step_k_one_launch_gpu.py holds that bar).  The width of the robot's ORCA group differs from the
// per-step form's (32 lanes here, the smallest instantiated size >= N + S there): lanes past the valid rows rank
// at +inf and are masked out of every ballot, so the width cannot change a result.
#pragma once

#include <type_traits>

#include "ebc_kernels.h"
#include "ebc_sail.h"

namespace ebc {

#define EBC_RO_THREADS 256
#define EBC_RO_WAVES (EBC_RO_THREADS / EBC_WAVE)
#define EBC_RO_RW 32       // lanes of the robot's ORCA group (check_robot_orca: N + S <= 32)
#define EBC_RO_MAX_EPG 16  // envs per workgroup, at most
#define EBC_RO_TMAX 17     // widest rotated row
// Waves per SIMD the register budget is set for = workgroups per CU.  Measured at 4096 x 10 (DESIGN.md section 3,
// item 15; GS = 9): without a budget the kernel takes 236 registers — the robot side (grid window, reward,
// double-precision policy) is the part that wants them; at 4 (128) it spills 93 of them to scratch and every
// workgroup of the launch is resident at once; at 5 and 6 (115 / 197 spilled) the step is slower again.
#ifndef EBC_RO_OCC
#define EBC_RO_OCC 4
#endif

struct RolloutIO {
  int K, robot_policy, auto_reset, epg;
  int T;  // floats per rotated row (13 or 17)
  double safety_space;
  RobotSim sim;
  const double *robot_action;
  float *state_rotated;
  long long *n_rows;
  double *robot_action_out, *reward;
  uint8_t *done, *info;
  double *dmin, *dist_to_goal;
  float *obs_rotated;
};

// Byte offsets of the workgroup's LDS arrays (each 16-byte aligned).  Host and device use the same function.
struct RolloutLds {
  unsigned hum;    // 9 arrays [epg * N] of double: px py vx vy gx gy radius v_pref arrival
  unsigned type;   // [epg * N] int
  unsigned tile;   // [2 * epg * N] float4 (DevState::tile layout)
  unsigned stat;   // 3 arrays [epg * S] of double: spx spy sradius
  unsigned robot, rn;  // [epg][9] double: current / next robot state
  unsigned act;        // [epg][2] double
  unsigned gtime, tnew;  // [epg] double
  unsigned dist;       // [epg * N] double: swept distances
  unsigned vel;        // [epg * N] float2: the humans' ORCA velocities
  unsigned ints;       // 7 arrays [epg] of int: n, ns, slot, cursor, done, sim_rows, restore
  unsigned sim_self;   // [epg] float2
  unsigned sim_radius;  // [epg * R] float
  unsigned frame_cur, frame_next;  // [epg] RotFrame: the robot-centric frame of the current / the next robot state
  unsigned rows_state, rows_obs;  // [epg * R * T] float each
  unsigned scratch, scratch_stride;  // EBC_RO_WAVES ORCA scratch areas
  unsigned bytes;
};
__host__ __device__ inline RolloutLds rollout_lds(int epg, int N, int S, int T, unsigned scratch_bytes) {
  RolloutLds L;
  unsigned o = 0;
  auto take = [&](unsigned bytes) {
    const unsigned at = o;
    o += (bytes + 15u) & ~15u;
    return at;
  };
  const unsigned HN = (unsigned)epg * N, R = (unsigned)(N + S);
  L.hum = take(9 * HN * 8);
  L.type = take(HN * 4);
  L.tile = take(2 * HN * 16);
  L.stat = take(3 * (unsigned)epg * (S ? S : 1) * 8);
  L.robot = take((unsigned)epg * 72);
  L.rn = take((unsigned)epg * 72);
  L.act = take((unsigned)epg * 16);
  L.gtime = take((unsigned)epg * 8);
  L.tnew = take((unsigned)epg * 8);
  L.dist = take(HN * 8);
  L.vel = take(HN * 8);
  L.ints = take(7 * (unsigned)epg * 4);
  L.sim_self = take((unsigned)epg * 8);
  L.sim_radius = take((unsigned)epg * R * 4);
  L.frame_cur = take((unsigned)epg * sizeof(RotFrame));
  L.frame_next = take((unsigned)epg * sizeof(RotFrame));
  L.rows_state = take((unsigned)epg * R * T * 4);
  L.rows_obs = take((unsigned)epg * R * T * 4);
  L.scratch_stride = (scratch_bytes + 15u) & ~15u;
  L.scratch = take(EBC_RO_WAVES * L.scratch_stride);
  L.bytes = o;
  return L;
}

template <int GS>
struct RolloutScratch {
  static constexpr unsigned A = (unsigned)OrcaLds<GS>::BYTES, B = (unsigned)OrcaLds<EBC_RO_RW>::BYTES;
  static constexpr unsigned BYTES = A > B ? A : B;
};

// A row in frame f (or zeros) into an LDS row buffer: the first T floats of it
__device__ __forceinline__ void rollout_put_row(float *dst, const RotFrame &f, const ObsRow &row, int T) {
  float out[EBC_RO_TMAX];
  rotated_row_or_zeros<EBC_RO_TMAX>(f, row, out);
#pragma unroll
  for (int c = 0; c < EBC_RO_TMAX; ++c)
    if (c < T) dst[c] = out[c];
}

// EBC_ROBOT_SAIL: the attached network (ebc_robot_sail) and how many envs go through its LDS area at a time
struct RolloutSail {
  const float *P;  // the packed weight image (ebc_sail_rule.h), device
  int N;           // adult_num
  int chunk;       // envs per pass of the network: min(epg, group_envs(N)), fewer when LDS is short
};

// Inputs of sail_group (ebc_sail.h) from the rollout kernel's LDS state: the rows ebc_observe's `ob` would hold
// (obs_row), cast once.
struct RolloutSailSrc {
  const double *robot_base;
  EnvRows<int> rows;  // of the workgroup
  const int *n_h, *n_s;
  int N, S, el0;
  __device__ __forceinline__ const double *robot(int g) const { return robot_base + (el0 + g) * 9; }
  __device__ __forceinline__ float frame(int g, int i, int c) const {
    const int el = el0 + g;
    const ObsRow o = obs_row(rows.at(el * N, el * S), i, n_h[el], n_s[el]);
    return (float)(c == 0 ? o.px : c == 1 ? o.py : c == 2 ? o.vx : o.vy);
  }
};

// The kernel's third argument: RolloutIO, and with EBC_ROBOT_SAIL the network behind it
struct RolloutIOSail : RolloutIO {
  RolloutSail sail;
};
template <bool SAIL>
using RolloutArg = typename std::conditional<SAIL, RolloutIOSail, RolloutIO>::type;

// ebc_step_k_world: the records of the world before every step, [K][E][9] and [K][E][R][5] doubles; either may be null
struct RolloutWorld {
  double *robot, *ob;
};
template <bool SAIL>
struct RolloutIOWorld : RolloutArg<SAIL> {
  RolloutWorld world;
};
template <bool SAIL, bool WORLD>
using RolloutArgW = typename std::conditional<WORLD, RolloutIOWorld<SAIL>, RolloutArg<SAIL>>::type;

// `cnt` doubles, value(f) for f in [0, cnt), -> dst in flat order, by THREADS threads: 16-byte stores from the first
// 16-byte boundary of the destination on, a single double before and behind (flush_rows' shape, for doubles that are
// computed from the LDS state instead of lying in a buffer).
template <int THREADS, typename F>
__device__ __forceinline__ void world_store(double *dst, int cnt, int tid, F value) {
  int head = (int)(((size_t)dst >> 3) & 1);
  head = head < cnt ? head : cnt;
  if (tid < head) dst[tid] = value(tid);
  const int body2 = (cnt - head) / 2;
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  for (int v = tid; v < body2; v += THREADS) {
    const int f = head + 2 * v;
    const f64x2 w = {value(f), value(f + 1)};
    *reinterpret_cast<f64x2 *>(dst + f) = w;
  }
  const int tail0 = head + 2 * body2;
  if (tid < cnt - tail0) dst[tail0 + tid] = value(tail0 + tid);
}

// SAIL = false is the kernel of the three robot policies as it was measured; SAIL = true (EBC_ROBOT_SAIL) is an
// instantiation of its own, so that theirs keeps its register allocation: it adds the network's decision in P1 and
// nothing anywhere else.
// MIXED = true is EBC_HUMAN_BY_TYPE's instantiation (csrc/ebcsim_mix.hip), again one of its own: the group of a human on
// the linear policy idles through the ORCA pass, and the human's commit in P3a takes linear_policy of the pre-step state,
// which is still in LDS there, in place of vel[].  Nothing else differs.
// WORLD = true is ebc_step_k_world's (csrc/ebcsim_world.hip), one more of its own for the same reason: at the top of P1
// all threads write the robot array and the world-frame rows of the workgroup's envs from LDS, the values the SAIL
// source struct reads there.  A workgroup's envs are consecutive, so each record of a step is one contiguous run of
// envs * 9 and envs * R * 5 doubles.  No LDS of its own.
template <int GS, bool SAIL = false, bool MIXED = false, bool WORLD = false>
__global__ __launch_bounds__(EBC_RO_THREADS, EBC_RO_OCC) void rollout_kernel(EbcParams p, DevState s, RolloutArgW<SAIL, WORLD> io) {
  extern __shared__ __align__(16) unsigned char ro_lds[];
  const int tid = threadIdx.x, lane = tid & (EBC_WAVE - 1), wave = tid / EBC_WAVE;
  const int N = s.N, S = s.S, R = N + S, EPG = io.epg, T = io.T, E = s.E;
  const int e0 = (int)blockIdx.x * EPG;
  const int envs = min(EPG, E - e0);  // the last workgroup may own fewer
  const int HN = envs * N, SN = envs * S, RN = envs * R;
  const RolloutLds L = rollout_lds(EPG, N, S, T, RolloutScratch<GS>::BYTES);
  double *const hum = reinterpret_cast<double *>(ro_lds + L.hum);
  const int HS = EPG * N;  // stride between the human arrays
  double *const h_px = hum, *const h_py = hum + HS, *const h_vx = hum + 2 * HS, *const h_vy = hum + 3 * HS;
  double *const h_gx = hum + 4 * HS, *const h_gy = hum + 5 * HS, *const h_rad = hum + 6 * HS, *const h_vpref = hum + 7 * HS;
  double *const h_arr = hum + 8 * HS;
  int *const h_type = reinterpret_cast<int *>(ro_lds + L.type);
  float4 *const tile = reinterpret_cast<float4 *>(ro_lds + L.tile);
  const int SS = EPG * (S ? S : 1);
  double *const st_x = reinterpret_cast<double *>(ro_lds + L.stat), *const st_y = st_x + SS, *const st_r = st_x + 2 * SS;
  double *const robot = reinterpret_cast<double *>(ro_lds + L.robot);
  double *const robot_next = reinterpret_cast<double *>(ro_lds + L.rn);
  double *const act = reinterpret_cast<double *>(ro_lds + L.act);
  double *const gtime = reinterpret_cast<double *>(ro_lds + L.gtime);
  double *const tnew = reinterpret_cast<double *>(ro_lds + L.tnew);
  double *const dist = reinterpret_cast<double *>(ro_lds + L.dist);
  float2 *const vel = reinterpret_cast<float2 *>(ro_lds + L.vel);
  int *const n_h = reinterpret_cast<int *>(ro_lds + L.ints), *const n_s = n_h + EPG, *const slot = n_h + 2 * EPG;
  int *const cursor = n_h + 3 * EPG, *const done = n_h + 4 * EPG, *const sim_rows = n_h + 5 * EPG, *const restore = n_h + 6 * EPG;
  float2 *const sim_self = reinterpret_cast<float2 *>(ro_lds + L.sim_self);
  float *const sim_radius = reinterpret_cast<float *>(ro_lds + L.sim_radius);
  RotFrame *const frame_cur = reinterpret_cast<RotFrame *>(ro_lds + L.frame_cur);
  RotFrame *const frame_next = reinterpret_cast<RotFrame *>(ro_lds + L.frame_next);
  float *const rows_state = reinterpret_cast<float *>(ro_lds + L.rows_state);
  float *const rows_obs = reinterpret_cast<float *>(ro_lds + L.rows_obs);
  unsigned char *const scratch = ro_lds + L.scratch + (unsigned)wave * L.scratch_stride;
  const ScenePool &P = s.pool;
  const double dt = p.time_step;
  const bool robot_orca = io.robot_policy == EBC_ROBOT_ORCA;
  // the LDS state as the shared rules take it (el in place of the env index)
  const EnvRows<int> lds_rows = {h_px, h_py, h_vx, h_vy, h_rad, h_type, st_x, st_y, st_r};
  const RobotSim lds_sim = {io.sim.rows ? sim_rows : nullptr, sim_radius, sim_self};
  const OrcaHot lds_hot = {E, N, s.n_magic, s.n_shift, tile, n_h};

  // ---- the envs' state: global memory -> LDS, once
  for (int q = tid; q < HN; q += EBC_RO_THREADS) {
    const size_t k = (size_t)e0 * N + q;
    h_px[q] = s.px[k]; h_py[q] = s.py[k]; h_vx[q] = s.vx[k]; h_vy[q] = s.vy[k];
    h_gx[q] = s.gx[k]; h_gy[q] = s.gy[k]; h_rad[q] = s.radius[k]; h_vpref[q] = s.v_pref[k];
    h_arr[q] = s.arrival[k];
    h_type[q] = s.type[k];
    tile[2 * q] = s.tile[2 * k];
    tile[2 * q + 1] = s.tile[2 * k + 1];
  }
  for (int q = tid; q < SN; q += EBC_RO_THREADS) {
    const size_t k = (size_t)e0 * S + q;
    st_x[q] = s.spx[k]; st_y[q] = s.spy[k]; st_r[q] = s.sradius[k];
  }
  for (int q = tid; q < envs * 9; q += EBC_RO_THREADS) robot[q] = s.robot[(size_t)e0 * 9 + q];
  if (tid < envs) {
    const size_t e = (size_t)e0 + tid;
    gtime[tid] = s.time[e];
    n_h[tid] = s.n_humans[e];
    n_s[tid] = S ? s.n_static[e] : 0;
    slot[tid] = s.grid_scene[e];
    cursor[tid] = P.P > 0 ? P.cursor[e] : (int)e;  // without a custom pool an env restarts from its own slot
    done[tid] = s.done[e];
    if (io.sim.rows) {
      sim_rows[tid] = io.sim.rows[e];
      sim_self[tid] = io.sim.self[e];
    }
  }
  if (io.sim.rows)
    for (int q = tid; q < RN; q += EBC_RO_THREADS) sim_radius[q] = io.sim.radius[(size_t)e0 * R + q];
  __syncthreads();
  if (io.state_rotated) {
    if (tid < envs) frame_cur[tid] = rot_frame(robot + tid * 9, p.rotate_unicycle);
    __syncthreads();
  }

  const int human_passes = (HN + (EBC_WAVE / GS) - 1) / (EBC_WAVE / GS);
  const int robot_passes = robot_orca ? (envs + (EBC_WAVE / EBC_RO_RW) - 1) / (EBC_WAVE / EBC_RO_RW) : 0;

  // The robot side of a step runs on the LAST wave (its ORCA groups or its policy, swept distances, reduce, grid window,
  // reward): it needs nothing from the humans' ORCA, so it meets the other waves only at the barrier before the commit.
  // The humans' ORCA passes are dealt out to all waves when the robot's action is cheap, to the others when it is ORCA.
  const int orca_waves = robot_orca && EBC_RO_WAVES > 1 ? EBC_RO_WAVES - 1 : EBC_RO_WAVES;

  for (int k = 0; k < io.K; ++k) {
    const size_t ke = (size_t)k * E + e0;  // first env of this workgroup in a [K][E] output
    // ================================================================ P1
    if (k > 0 && io.obs_rotated) flush_rows<EBC_RO_THREADS>(rows_obs, io.obs_rotated + (ke - E) * R * T, RN * T, tid);
    if constexpr (WORLD) {  // ebc_get_state's robot and ebc_observe's ob of the state before step k
      if (io.world.robot) world_store<EBC_RO_THREADS>(io.world.robot + ke * 9, envs * 9, tid, [&](int f) { return robot[f]; });
      if (io.world.ob)
        world_store<EBC_RO_THREADS>(io.world.ob + ke * R * 5, RN * 5, tid, [&](int f) {
          const int el = f / (R * 5), rem = f - el * (R * 5), r = rem / 5, c = rem - r * 5;
          const ObsRow o = obs_row(lds_rows.at(el * N, el * S), r, n_h[el], n_s[el]);
          return c == 0 ? o.px : c == 1 ? o.py : c == 2 ? o.vx : c == 3 ? o.vy : o.radius;
        });
    }
    if (io.state_rotated) {  // rows of the current state in the robot's frame
      for (int q = tid; q < RN; q += EBC_RO_THREADS) {
        const int el = q / R, r = q - el * R;
        rollout_put_row(rows_state + (size_t)q * T, frame_cur[el], obs_row(lds_rows.at(el * N, el * S), r, n_h[el], n_s[el]), T);
      }
    }
    if constexpr (SAIL) {
      // The network's decision from the LDS state, on all four waves, a chunk of envs at a time; the action goes to
      // act[] as the per-step form's sail_kernel would have written it.  The last wave reads act[] behind the barrier.
      const SailLds SL = sail_lds(reinterpret_cast<float *>(ro_lds + L.bytes), io.sail.chunk, io.sail.N);
      for (int c0 = 0; c0 < envs; c0 += io.sail.chunk) {
        const int ne = min(io.sail.chunk, envs - c0);
        const RolloutSailSrc src = {robot, lds_rows, n_h, n_s, N, S, c0};
        sail_group<EBC_RO_WAVES>(io.sail.P, io.sail.N, SL, ne, src);
        const float *planned = SL.planned();
        for (int q = tid; q < ne * 2; q += EBC_RO_THREADS) {
          const int g = q >> 1, c = q & 1, el = c0 + g;
          const bool rows_ok = n_h[el] + n_s[el] == io.sail.N;
          act[2 * el + c] = ebc_sail::action_of(planned[g * EBC_SAIL_HIDDEN + c], ebc_sail::arrived(robot + el * 9), rows_ok);
        }
        // the next chunk's first store to `planned` lies behind two barriers of sail_group
      }
      __syncthreads();
    }
    if (wave == EBC_RO_WAVES - 1) {
      if (lane < envs && io.n_rows) io.n_rows[ke + lane] = (long long)n_h[lane] + n_s[lane];
      if (robot_orca) {
        for (int pass = 0; pass < robot_passes; ++pass) {  // orca_robot_kernel's solve: lane, robot, row and simulator from LDS
          RobotLane l;
          l.group = lane / EBC_RO_RW;
          l.j = lane - l.group * EBC_RO_RW;
          const int el = pass * (EBC_WAVE / EBC_RO_RW) + l.group;
          l.e_ok = el < envs;
          l.ee = l.e_ok ? (size_t)el : 0;
          l.n = l.e_ok ? n_h[l.ee] : 0;
          l.ns = l.e_ok ? n_s[l.ee] : 0;
          const ObsRow row = obs_row(lds_rows.at(l.ee * N, l.ee * S), l.j, l.n, l.ns);
          float ox, oy;
          orca_robot_solve<EBC_RO_RW>(p, s, io.safety_space, lds_sim, scratch, l, robot + l.ee * 9, row, ox, oy);
          if (l.e_ok && l.j == 0) {
            act[2 * l.ee] = (double)ox;  // getAgentVelocity -> Python float
            act[2 * l.ee + 1] = (double)oy;
          }
        }
      } else if (!SAIL && lane < envs) {
        double a0, a1;
        robot_action(io.robot_policy, io.robot_action, ke + lane, robot + lane * 9, a0, a1);
        act[2 * lane] = a0;
        act[2 * lane + 1] = a1;
      }
      wave_sync();  // act
      for (int q = lane; q < HN; q += EBC_WAVE) {  // collisions.py:29-57 with the humans' CURRENT velocity
        const int el = q / N, i = q - el * N;
        const double *rb = robot + el * 9;
        const double a0 = act[2 * el], a1 = act[2 * el + 1];
        double rvx, rvy;
        swept_robot_velocity(p.robot_kinematics, a0, a1, rb[8], rvx, rvy);
        dist[q] = i < n_h[el] ? closest_dist(h_px[q], h_py[q], h_vx[q], h_vy[q], h_rad[q], rb[0], rb[1], rb[4], rvx, rvy, dt) : 0.0;
      }
      wave_sync();  // dist
      if (lane < envs) {
        const int el = lane;
        double rb[9], rn[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) rn[c] = rb[c] = robot[el * 9 + c];
        const double a0 = act[2 * el], a1 = act[2 * el + 1];
        robot_advance(p, rn, a0, a1);
        TypeWalk w;  // env_lane_role's walk and ordered combination of its quarters, as one walk
        for (int i = 0, n = n_h[el]; i < n; ++i) w.visit(dist[el * N + i], h_type[el * N + i]);
        int c4[4] = {w.coll[0], w.coll[1], w.coll[2], 0};
        c4[3] = grid_collision(P.grid ? P.grid + (size_t)slot[el] * s.G * 2 : nullptr, s.G, p.map_size_m, p.map_resolution,
                               rn[0], rn[1], rb[4], nullptr);
        const double g_now = gtime[el];
        const RewardOut ro = reward_compute(p, rn[0], rn[1], rb[5], rb[6], rb[4], a1, g_now, w.dmin, c4);
        store_outcome(io, ke + el, ro, w.dmin, a0, a1);
#pragma unroll
        for (int c = 0; c < 9; ++c) robot_next[el * 9 + c] = rn[c];
        if (io.obs_rotated || io.state_rotated) frame_next[el] = rot_frame(rn, p.rotate_unicycle);
        done[el] = ro.done;
        restore[el] = (io.auto_reset && ro.done) ? 1 : 0;
        tnew[el] = g_now + dt;
      }
    }
    for (int hp = 0; hp < human_passes; ++hp) {  // the humans' ORCA, tile and robot from LDS
      if (hp % orca_waves != wave) continue;
      constexpr int HPW = EBC_WAVE / GS;
      const int group = lane / GS, j = lane - group * GS;
      const int u = hp * HPW + group;           // human of this workgroup: el * N + i
      const bool h_ok = group < HPW && u < HN;  // lanes past HPW * GS idle
      const int el = h_ok ? u / N : 0;
      const int i = h_ok ? u - el * N : 0;
      bool solve = h_ok;
      if constexpr (MIXED) solve = h_ok && !human_on_linear(s, h_type[h_ok ? u : 0]);
      const OrcaTile t = orca_tile_load<GS>(lds_hot, solve, el, i);
      float ox, oy;
      bool human_ok;
      orca_wave_compute<GS>(p, s, N, t, [&] { return robot + el * 9; }, solve, i, scratch, ox, oy, human_ok);
      if (h_ok && j == 0) vel[u] = make_float2(human_ok ? ox : 0.0f, human_ok ? oy : 0.0f);
    }
    __syncthreads();
    // ================================================================ P3a
    if (io.state_rotated) flush_rows<EBC_RO_THREADS>(rows_state, io.state_rotated + ke * R * T, RN * T, tid);
    bool any_restore = false;
    for (int el = 0; el < envs; ++el) any_restore = any_restore || restore[el];  // the same answer in every thread
    for (int q = tid; q < HN; q += EBC_RO_THREADS) {
      const int el = q / N, i = q - el * N;
      if (i >= n_h[el]) continue;
      // Agent.step (agent.py:202-211), first arrival (env.py:365-378), the float tile record (orca.py:110-140):
      // state_role's commit; the row is rows_role's
      double ax = (double)vel[q].x, ay = (double)vel[q].y;  // getAgentVelocity -> Python float
      if constexpr (MIXED) {
        if (human_on_linear(s, h_type[q])) linear_policy(h_px[q], h_py[q], h_gx[q], h_gy[q], h_vpref[q], ax, ay);  // env.py:393-405
      }
      const double px = h_px[q] + ax * dt, py = h_py[q] + ay * dt;
      const double rad = h_rad[q];
      if (io.obs_rotated)
        rollout_put_row(rows_obs + (size_t)(el * R + i) * T, frame_next[el], ObsRow{px, py, ax, ay, rad, h_type[q], true}, T);
      if (!restore[el]) {
        const double dx = h_gx[q] - px, dy = h_gy[q] - py;
        const double dg = norm2(dx, dy);
        if (h_arr[q] == 0 && dg < rad) h_arr[q] = tnew[el];
        float prefx, prefy;
        orca_pref_from(dx, dy, dg, prefx, prefy);
        h_px[q] = px; h_py[q] = py; h_vx[q] = ax; h_vy[q] = ay;
        tile[2 * q] = make_float4((float)px, (float)py, (float)ax, (float)ay);
        tile[2 * q + 1] = make_float4((float)(rad + 0.01 + p.orca_safety_space), (float)h_vpref[q], prefx, prefy);
      }
    }
    if (io.obs_rotated) {  // static obstacles as pedestrians (env.py:457-458) and the padding rows
      for (int q = tid; q < RN; q += EBC_RO_THREADS) {
        const int el = q / R, r = q - el * R;
        const int n = n_h[el];
        if (r < n) continue;  // a human's row: above, moved
        rollout_put_row(rows_obs + (size_t)q * T, frame_next[el], obs_row(lds_rows.at(el * N, el * S), r, n, n_s[el]), T);
      }
    }
    if (tid < envs) {
      if (!restore[tid]) {
#pragma unroll
        for (int c = 0; c < 9; ++c) robot[tid * 9 + c] = robot_next[tid * 9 + c];
        gtime[tid] = tnew[tid];
        if (io.state_rotated) frame_cur[tid] = frame_next[tid];  // rot_frame of the same nine doubles
      } else {
        slot[tid] = cursor[tid];  // the scene the env restarts from, and its occupancy grid from now on
      }
    }
    // ================================================================ P3b: restart scenes (rare)
    // state_role's restore branch: every per-scene field from the pool slot, time 0, the cursor walks on
    if (any_restore) {
      __syncthreads();  // the rows above read the pre-step rows and row counts
      for (int q = tid; q < HN; q += EBC_RO_THREADS) {
        const int el = q / N, i = q - el * N;
        if (!restore[el]) continue;
        const RestartHuman h = restart_human(p, P, N, slot[el], i);
        h_px[q] = h.px; h_py[q] = h.py; h_vx[q] = h.vx; h_vy[q] = h.vy;
        h_gx[q] = h.gx; h_gy[q] = h.gy; h_rad[q] = h.radius; h_vpref[q] = h.v_pref;
        h_arr[q] = 0.0;
        h_type[q] = h.type;
        tile[2 * q] = h.tile0;
        tile[2 * q + 1] = h.tile1;
      }
      for (int q = tid; q < SN; q += EBC_RO_THREADS) {
        const int el = q / S, r = q - el * S;
        if (!restore[el]) continue;
        const size_t src = (size_t)slot[el] * S + r;
        st_x[q] = P.spx[src]; st_y[q] = P.spy[src]; st_r[q] = P.sradius[src];
      }
      if (tid < envs && restore[tid]) {
        const int cur = slot[tid];
        n_h[tid] = P.n_humans[cur];
        if (S) n_s[tid] = P.n_static[cur];
#pragma unroll
        for (int c = 0; c < 9; ++c) robot[tid * 9 + c] = P.robot[(size_t)cur * 9 + c];
        gtime[tid] = 0.0;
        if (io.state_rotated) frame_cur[tid] = rot_frame(robot + tid * 9, p.rotate_unicycle);
        if (P.P > 0) cursor[tid] = pool_next_cursor(P, E, cur);  // without a custom pool the env keeps restarting from its own slot
      }
    }
    __syncthreads();
  }
  if (io.obs_rotated) flush_rows<EBC_RO_THREADS>(rows_obs, io.obs_rotated + ((size_t)(io.K - 1) * E + e0) * R * T, RN * T, tid);

  // ---- LDS -> global memory, once: what K per-step steps would have left
  for (int q = tid; q < HN; q += EBC_RO_THREADS) {
    const size_t k = (size_t)e0 * N + q;
    s.px[k] = h_px[q]; s.py[k] = h_py[q]; s.vx[k] = h_vx[q]; s.vy[k] = h_vy[q];
    s.gx[k] = h_gx[q]; s.gy[k] = h_gy[q]; s.radius[k] = h_rad[q]; s.v_pref[k] = h_vpref[q];
    s.arrival[k] = h_arr[q];
    s.type[k] = (uint8_t)h_type[q];
    s.tile[2 * k] = tile[2 * q];
    s.tile[2 * k + 1] = tile[2 * q + 1];
  }
  for (int q = tid; q < SN; q += EBC_RO_THREADS) {
    const size_t k = (size_t)e0 * S + q;
    s.spx[k] = st_x[q]; s.spy[k] = st_y[q]; s.sradius[k] = st_r[q];
  }
  for (int q = tid; q < envs * 9; q += EBC_RO_THREADS) s.robot[(size_t)e0 * 9 + q] = robot[q];
  if (tid < envs) {
    const size_t e = (size_t)e0 + tid;
    s.time[e] = gtime[tid];
    s.n_humans[e] = n_h[tid];
    if (S) s.n_static[e] = n_s[tid];
    s.grid_scene[e] = slot[tid];
    if (P.P > 0) P.cursor[e] = cursor[tid];
    s.done[e] = (uint8_t)done[tid];
    if (io.sim.rows) {
      io.sim.rows[e] = sim_rows[tid];
      io.sim.self[e] = sim_self[tid];
    }
  }
  if (io.sim.rows)
    for (int q = tid; q < RN; q += EBC_RO_THREADS) io.sim.radius[(size_t)e0 * R + q] = sim_radius[q];
}

}  // namespace ebc
