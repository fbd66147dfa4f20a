// ebc_orca_wide.h — the robot's own ORCA solve (orca_robot_kernel, ebc_kernels.h) on observations of 33 .. 128 rows.
//
// orca_robot_kernel gives one lane of a group to each row, so it ends with the widest group, 32 lanes.  RVO2 never uses
// more than maxNeighbors = 10 rows of however many there are: Agent::insertAgentNeighbor keeps the 10 nearest in range.
// A wider observation therefore changes WHICH rows enter the solve, not the solve.  Here a 32-lane half of a wave serves
// one env in two phases:
//   select   lane j owns rows j, j + 32, j + 64, j + 96 of the observation (obs_row of env_rows, as the narrow kernel
//            reads them), casts them as orca_robot_solve does, ranks every in-range row among ALL rows of the env by
//            (distSq, row index) through LDS, and writes the rows of rank < min(maxNeighbors, EBC_MAXNB) to LDS at
//            their rank: position, velocity, radius, as float.
//   solve    orca_group<32>, unchanged: lane j < nn describes the row of rank j.  Its own ranking of rows that stand in
//            ranked order already is the identity (equal distances stay in row order, which is their order here), so
//            lines, linearProgram2 / 3 and the result are those of the scalar RVO2 form on the full list of rows.
// An env never leaves its wave, so wave_sync() (ebc_orca_group.h) orders the LDS traffic, and the persistent
// simulator's read-before-replace of sim.rows[e] holds as in orca_robot_solve: every lane has read the row count before
// lane 0 of the half replaces it.
#pragma once

#include "ebc_kernels.h"

namespace ebc {

#define EBC_OW_LANES 32                                // lanes that serve one env: the widest ORCA group
#define EBC_OW_ROWS 128                                // ebc_create: max_humans + max_static <= 128
#define EBC_OW_SLOTS (EBC_OW_ROWS / EBC_OW_LANES)      // rows a lane owns
#define EBC_OW_ENVS (EBC_WAVE / EBC_OW_LANES)          // envs per wave (= per workgroup)

// LDS of one workgroup: orca_group's scratch, then per env the distances of all rows and the selected rows
struct OrcaWideLds {
  unsigned char scratch[OrcaLds<EBC_OW_LANES>::BYTES];
  float dist[EBC_OW_ENVS][EBC_OW_ROWS];
  float4 pv[EBC_OW_ENVS][EBC_MAXNB];   // position, velocity of the row of rank k
  float rad[EBC_OW_ENVS][EBC_MAXNB + 2];
};

static __global__ __launch_bounds__(EBC_WAVE) void orca_robot_wide_kernel(EbcParams p, DevState s, double safety_space, double *act,
                                                                          RobotSim sim) {
  constexpr int GS = EBC_OW_LANES;
  using L = OrcaLds<GS>;
  __shared__ __align__(16) unsigned char lds_bytes[sizeof(OrcaWideLds)];
  OrcaWideLds &lds = *reinterpret_cast<OrcaWideLds *>(lds_bytes);
  const RobotLane l = robot_lane<GS>(s);  // idle lanes (no env): e_ok false, ee = 0, no row exists
  const int group = l.group, j = l.j, n = l.n, ns = l.ns;
  const size_t ee = l.ee;
  const int R = s.N + s.S;
  const double *rb = s.robot + ee * 9;
  const float posx = (float)rb[0], posy = (float)rb[1], velx = (float)rb[2], vely = (float)rb[3];
  float radius = (float)(rb[4] + 0.01 + safety_space), maxSpeed = (float)rb[7];
  float prefx, prefy;
  orca_pref_velocity(rb[0], rb[1], rb[5], rb[6], prefx, prefy);
  const int maxN = p.orca_max_neighbors < EBC_MAXNB ? p.orca_max_neighbors : EBC_MAXNB;

  // ---- select: this lane's rows, as rvo2 holds them
  const EnvRows<uint8_t> rows = env_rows(s, ee);
  float opx[EBC_OW_SLOTS], opy[EBC_OW_SLOTS], ovx[EBC_OW_SLOTS], ovy[EBC_OW_SLOTS], orad[EBC_OW_SLOTS], d[EBC_OW_SLOTS];
  bool valid[EBC_OW_SLOTS], inRange[EBC_OW_SLOTS];
  float *dist = lds.dist[group];
#pragma unroll
  for (int t = 0; t < EBC_OW_SLOTS; ++t) {
    const int r = j + t * GS;
    opx[t] = opy[t] = ovx[t] = ovy[t] = orad[t] = 0.0f;
    valid[t] = false;
    if (t * GS < R) {  // kernel-uniform
      const ObsRow row = obs_row(rows, r, n, ns);
      valid[t] = row.valid;
      if (row.valid) {  // a static row's velocity is the 0 obs_row gave it
        opx[t] = (float)row.px;
        opy[t] = (float)row.py;
        ovx[t] = (float)row.vx;
        ovy[t] = (float)row.vy;
        orad[t] = (float)(row.radius + 0.01 + safety_space);
      }
    }
    // Agent::insertAgentNeighbor, the arithmetic of orca_group
    const float ddx = posx - opx[t], ddy = posy - opy[t];
    d[t] = ddx * ddx + ddy * ddy;
    inRange[t] = valid[t] && d[t] < s.range_sq;
    dist[r] = inRange[t] ? d[t] : INFINITY;  // r < EBC_OW_ROWS: rows past R count for nobody
  }
  bool rebuild = true;
  if (sim.rows && l.e_ok) {
    // every lane of the half reads the simulator's row count before lane 0 replaces it (one wave)
    rebuild = sim.rows[ee] != n + ns;  // sim is None, or getNumAgents() != len(agent_states) + 1
    if (rebuild) {
#pragma unroll
      for (int t = 0; t < EBC_OW_SLOTS; ++t)
        if (valid[t]) sim.radius[ee * (size_t)R + j + t * GS] = orad[t];
      if (j == 0) {
        sim.self[ee] = make_float2(radius, maxSpeed);
        sim.rows[ee] = n + ns;
      }
    } else {
      const float2 me = sim.self[ee];
      radius = me.x;
      maxSpeed = me.y;
    }
  }
  wave_sync();
  // rank = #{k : d_k < d or (d_k == d and k < row)} over all rows of the env
  int rank[EBC_OW_SLOTS];
#pragma unroll
  for (int t = 0; t < EBC_OW_SLOTS; ++t) rank[t] = 0;
  for (int k4 = 0; k4 * 4 < R; ++k4) {  // R <= EBC_OW_ROWS; the float4 that holds row R - 1 ends inside dist[]
    const float4 d4 = reinterpret_cast<const float4 *>(dist)[k4];
    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k4 * 4 + c;
#pragma unroll
      for (int t = 0; t < EBC_OW_SLOTS; ++t) rank[t] += (dv[c] < d[t] || (dv[c] == d[t] && k < j + t * GS)) ? 1 : 0;
    }
  }
  // compaction: the included rows at their rank
  int nn = 0;
#pragma unroll
  for (int t = 0; t < EBC_OW_SLOTS; ++t) {
    const bool included = inRange[t] && rank[t] < maxN;
    nn += __popc(group_ballot<GS>(included, group));
    if (included) {
      float rad = orad[t];
      if (!rebuild) rad = sim.radius[ee * (size_t)R + j + t * GS];  // the radius of the call that built the simulator
      lds.pv[group][rank[t]] = make_float4(opx[t], opy[t], ovx[t], ovy[t]);
      lds.rad[group][rank[t]] = rad;
    }
  }
  wave_sync();

  // ---- solve: lane j < nn describes the row of rank j
  const bool sel = j < nn;
  float qpx = 0, qpy = 0, qvx = 0, qvy = 0, qrad = 0;
  if (sel) {
    const float4 q = lds.pv[group][j];
    qpx = q.x;
    qpy = q.y;
    qvx = q.z;
    qvy = q.w;
    qrad = lds.rad[group][j];
  }
  float *dist_lds;
  float4 *lines_lds, *segs_lds, *proj_lds;
  orca_scratch_carve<GS>(lds.scratch, dist_lds, lines_lds, segs_lds, proj_lds);
  float ox, oy;
  orca_group<GS>(p, j, group, sel, posx, posy, velx, vely, radius, maxSpeed, prefx, prefy, qpx, qpy, qvx, qvy, qrad,
                 dist_lds + group * L::Sh::DIST, lines_lds + group * L::Sh::LINES, segs_lds + group * L::Sh::LINES,
                 proj_lds + group * L::Sh::LINES, maxN, s.range_sq, s.inv_time_horizon, s.inv_time_step, ox, oy);
  if (l.e_ok && j == 0) {
    act[2 * ee] = (double)ox;  // getAgentVelocity -> Python float
    act[2 * ee + 1] = (double)oy;
  }
}

}  // namespace ebc
