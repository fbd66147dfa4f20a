/*
 * ebcsim.h — C ABI of libebcsim.so, the MI355X-native batched crowd-navigation
 * simulator that replaces the simulation hot path of kolomeytsev/EB-CADRL.
 *
 * The reference has no FFI: its boundary is the duck-typed Python surface of
 * simulator/env.py (EntityBasedCollisionAvoidance).  Every entry point below
 * names the reference interface (file:line under the reference tree) it stands
 * in for.  The binding a maintainer of the reference would add is the ctypes
 * stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch types; every function returns EBC_OK (0) or a negative
 *     EbcStatus; the message of the last failure on the calling thread is
 *     ebc_last_error().
 *   - the caller owns every buffer it passes; the library owns the opaque
 *     handle and the device allocations behind it.
 *   - buffers are either all host or all device per call (`location`).  Host
 *     buffers are staged through the handle's own device buffers and the call
 *     returns after the copy-back; device buffers are used in place and the
 *     call only enqueues work on the handle's stream (ebc_synchronize waits).
 *   - batched layout is struct-of-arrays.  E = n_envs, N = max_humans (row
 *     stride of every per-human array, humans in the reference's type-major
 *     order adults, bicycles, children: simulator/env.py:393), S = max_static,
 *     R = N + S observation rows, T = 13 (+4 with agent type) rotated width.
 *   - simulator state is IEEE double (the reference keeps Python floats:
 *     simulator/agents/agent.py:164-228); ORCA runs in float exactly where the
 *     third-party rvo2 library does; rotated observations are float where the
 *     reference builds them with torch.Tensor (rl/policy/cadrl.py:236-337).
 *   - there is no CPU fallback: without a HIP device ebc_create fails.
 */
#ifndef EBCSIM_H
#define EBCSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EBC_ABI_VERSION 1

typedef enum EbcStatus {
  EBC_OK = 0,
  EBC_ERR_INVALID = -1,     /* bad argument (NULL, size, range)            */
  EBC_ERR_UNSUPPORTED = -2, /* valid in the reference, not built here      */
  EBC_ERR_DEVICE = -3,      /* HIP runtime error or no device              */
  EBC_ERR_STATE = -4        /* call order (e.g. step before reset)         */
} EbcStatus;

/* simulator/utils/utils.py:9-14 (AgentType) */
enum { EBC_ADULT = 0, EBC_BICYCLE = 1, EBC_CHILD = 2, EBC_ADULT_STATIC = 3, EBC_ROBOT = 4 };

/* Info subclass identity, simulator/utils/info.py, in the priority order of
 * Reward.compute (simulator/utils/reward.py:103-179). */
enum {
  EBC_INFO_NOTHING = 0,
  EBC_INFO_DANGER = 1,
  EBC_INFO_REACH_GOAL = 2,
  EBC_INFO_COLLISION_OBSTACLE = 3,
  EBC_INFO_COLLISION_ADULT = 4,
  EBC_INFO_COLLISION_BICYCLE = 5,
  EBC_INFO_COLLISION_CHILD = 6,
  EBC_INFO_TIMEOUT = 7
};

/* robot kinematics: Agent.kinematics (simulator/agents/agent.py:21, :164-188).
 * HOLONOMIC takes ActionXY(vx, vy); UNICYCLE takes ActionRot(v, r).  ActionXYRot
 * cannot pass compute_collision_agent_with_robot (simulator/utils/collisions.py
 * :41-42 reads action.v) and is therefore not part of the path. */
enum { EBC_HOLONOMIC = 0, EBC_UNICYCLE = 1 };

enum { EBC_HOST = 0, EBC_DEVICE = 1 };

/* who moves the humans this step (simulator/policy/policy_factory.py:10-14) */
enum {
  EBC_HUMAN_EXTERNAL = 0, /* velocities given by ebc_set_human_actions (BASELINE config 2) */
  EBC_HUMAN_LINEAR = 1,   /* simulator/policy/linear.py:17-23 */
  EBC_HUMAN_ORCA = 2,     /* simulator/policy/orca.py:85-157 (+ rvo2) */
  EBC_HUMAN_CACHED = 3,   /* re-use the velocities the last ebc_lookahead computed for the same state */
  EBC_HUMAN_BY_TYPE = 4   /* every entity type on its own policy (ebc_set_human_policies) */
};

enum {
  EBC_ROBOT_EXTERNAL = 0, /* robot_action[E][2] supplied */
  EBC_ROBOT_LINEAR = 1,   /* simulator/policy/linear.py:17-23 applied to the robot, on device */
  EBC_ROBOT_ORCA = 2,     /* ebc_step_k only: the robot on ORCA (ebc_robot_orca), the imitation-learning demonstrator */
  EBC_ROBOT_SAIL = 3      /* ebc_step_k only: the SAIL network attached with ebc_robot_sail decides every step */
};

/* flags */
enum {
  EBC_FLAG_AUTO_RESET = 1, /* a terminal step's outputs describe the terminal transition; the env's
                              state is then put back to its reset() scene (time 0) for the next step */
  EBC_FLAG_BORDER = 2,     /* border[4] valid: simulator/env.py:264-271 */
  EBC_FLAG_ONE_LAUNCH = 4  /* ebc_step_k: all K steps in ONE kernel launch, state kept on chip between steps */
};

/* Everything env.configure() / Reward.__init__ / ORCA.__init__ read from the INI
 * files (simulator/env.py:58-87, simulator/utils/reward.py:18-75,
 * simulator/policy/orca.py:58-69) plus the two policy-side switches rotate()
 * consults (rl/policy/cadrl.py:261, :304).  A missing optional key of the
 * reference (value None) is NaN here. */
typedef struct EbcParams {
  uint32_t struct_size; /* = sizeof(EbcParams), checked */
  int32_t robot_kinematics;
  int32_t robot_visible;     /* [robot] visible: humans see the robot (env.py:401-402) */
  int32_t new_reward;        /* reward.py:19 */
  double time_step;          /* [env] time_step */
  double time_limit;         /* [env] time_limit (getint) */
  double map_size_m;         /* [map] map_size_m */
  double map_resolution;     /* [map] map_resolution */
  double time_max;           /* reward.py:20 (NaN when absent) */
  double time_good;          /* reward.py:25 */
  double max_goal_distance;  /* reward.py:21 (NaN when absent: goal_reward None) */
  double success_reward;     /* reward.py:26 */
  double collision_penalty[4]; /* adult, bicycle, child, obstacle: reward.py:27-38 */
  double discomfort_dist[3];   /* adult, bicycle, child: reward.py:40-50 */
  double discomfort_factor[3]; /* adult, bicycle, child: reward.py:52-68 */
  double rotation_penalty_factor; /* reward.py:70 */
  double orca_safety_space;  /* orca.py:63 */
  float orca_neighbor_dist;  /* orca.py:64 */
  float orca_time_horizon;   /* orca.py:66 */
  int32_t orca_max_neighbors; /* orca.py:65 */
  int32_t with_agent_type;   /* sarl.py:103-110: T = 17 instead of 13 */
  int32_t rotate_unicycle;   /* policy kinematics == "unicycle": cadrl.py:261 */
  int32_t reserved;
} EbcParams;

/* Scene rows for ebc_reset: the outputs of SceneGenerator (simulator/scene/
 * scene_generator.py:330-378, :807-863) for n envs, all host pointers.
 * Per-human arrays are [n][N], per-static arrays [n][S], the grid is [n][G][2]
 * 64-bit words (G = round(map_size_m / map_resolution) <= 128): bit y of row x
 * set <=> scene.map[x, y] == 0 (occupied).  grid may be NULL (free map). */
typedef struct EbcScene {
  uint32_t struct_size;
  int32_t n;
  const int32_t *n_humans;   /* [n] */
  const double *px, *py, *vx, *vy, *gx, *gy, *radius, *v_pref; /* [n][N] */
  const uint8_t *type;       /* [n][N] AgentType 0..2.  The reference lays humans out type-major, but nothing here needs
                              * it: collisions and dmin walk each type's humans in index order whatever the layout,
                              * so interleaved types are accepted and give what the reference's per-type lists would */
  const int32_t *n_static;   /* [n] (may be NULL when S == 0) */
  const double *spx, *spy, *sradius; /* [n][S] static_obstacles_as_pedestrians */
  const uint64_t *grid;      /* [n][G][2] or NULL */
  const double *robot;       /* [n][9] px,py,vx,vy,radius,gx,gy,v_pref,theta (FullState order, state.py:1-12) */
} EbcScene;

/* One env.step(action, update=True) for every env (simulator/env.py:388-466). */
typedef struct EbcStepArgs {
  uint32_t struct_size;
  int32_t location;     /* of every pointer below */
  int32_t human_policy;
  int32_t robot_policy;
  int32_t flags;
  int32_t reserved;
  const double *robot_action; /* [E][2] ActionXY(vx,vy) or ActionRot(v,r); NULL with EBC_ROBOT_LINEAR */
  const double *border;       /* host [4] = x_lo, x_hi, y_lo, y_hi (always host) */
  /* outputs, each may be NULL */
  double *reward;       /* [E] */
  uint8_t *done;        /* [E] */
  uint8_t *info;        /* [E] EBC_INFO_* */
  double *dmin;         /* [E][3] dmin_adult, dmin_bicycle, dmin_child (inf when none) */
  double *dist_to_goal; /* [E] */
  double *robot_action_out; /* [E][2] the action applied (for EBC_ROBOT_LINEAR) */
  double *human_action; /* [E][N][2] velocities the humans chose this step */
  double *ob;           /* [E][R][5] px,py,vx,vy,radius of the returned ob list (env.py:381-382, :457-458) */
  float *obs_rotated;   /* [E][R][T] rotate(robot full state + ob row), cadrl.py:236-337 */
} EbcStepArgs;

/* The |A|-way env.onestep_lookahead sweep of MultiHumanRL.predict
 * (rl/policy/multi_human_rl.py:38-61) with humans evaluated once. */
typedef struct EbcLookaheadArgs {
  uint32_t struct_size;
  int32_t location;
  int32_t human_policy; /* LINEAR, ORCA or EXTERNAL */
  int32_t n_actions;    /* A */
  int32_t flags;
  int32_t reserved;
  const double *actions; /* [A][2], shared by all envs (cadrl.py:91-116) */
  const double *border;  /* host [4] or NULL */
  double *reward;        /* [E][A] */
  uint8_t *done;         /* [E][A] */
  uint8_t *info;         /* [E][A] */
  double *dmin;          /* [E][A][3] or NULL */
  double *next_ob;       /* [E][R][5] get_next_observable_state rows (env.py:449-458) or NULL */
  float *rows_rotated;   /* [E][A][R][T] rotate(propagate(robot, a) + next row) or NULL */
} EbcLookaheadArgs;

/* Read-back of the simulator state (env.states / Agent.get_full_state). */
typedef struct EbcStateView {
  uint32_t struct_size;
  int32_t location;
  double *px, *py, *vx, *vy, *gx, *gy, *radius, *v_pref; /* [E][N], each may be NULL */
  uint8_t *type;         /* [E][N] */
  int32_t *n_humans;     /* [E] */
  double *robot;         /* [E][9] FullState order */
  double *global_time;   /* [E] env.global_time */
  double *arrival_time;  /* [E][N] adult_times / bicycle_times / children_times (env.py:365-378) */
  uint8_t *done;         /* [E] latched terminal flag */
} EbcStateView;

int ebc_abi_version(void);
const char *ebc_last_error(void);

/* Defaults of the reference (ORCA constants orca.py:58-69, time_good reward.py:25). */
int ebc_params_default(EbcParams *p);

/* gym.make + env.configure + env.set_robot: simulator/__init__.py:4-7,
 * simulator/env.py:58-92.  Allocates device state for E envs on HIP device
 * `device_id`. */
int ebc_create(int device_id, int n_envs, int max_humans, int max_static,
               const EbcParams *params, void **handle_out);
int ebc_destroy(void *handle);

/* Run the handle's work on an existing HIP stream (e.g. torch's current
 * stream) so the caller's events order with it.  NULL is the HIP null stream
 * (torch's default stream).  Until this is called the handle uses a private
 * non-blocking stream created by ebc_create. */
int ebc_set_stream(void *handle, void *hip_stream);
int ebc_synchronize(void *handle);

/* env.reset for the listed envs (simulator/env.py:128-205): uploads the scene
 * rows, zeroes global_time and arrival times (env.py:149-151) and keeps a copy
 * for EBC_FLAG_AUTO_RESET.  env_ids NULL = envs 0..n-1. */
int ebc_reset(void *handle, const int32_t *env_ids, const EbcScene *scene);

/* Device-resident scene pool for EBC_FLAG_AUTO_RESET (the reference generates a fresh scene at
 * every env.reset on the host, simulator/scene/scene_generator.py:330-378; with thousands of envs
 * resets would dominate).  `pool` holds P host-generated scenes (same layout as for ebc_reset,
 * scene.n = P).  Env e restarts from scene cursor[e] = e mod P, and the cursor then advances by
 * `stride` (mod P), entirely on the device.  Without this call the pool is the envs' own
 * ebc_reset scenes (P = E, stride 0).  May be called again while episodes run (a smaller, larger
 * or regenerated pool): running episodes are not touched — an env that is in the middle of an
 * episode on a scene of the OLD pool keeps that scene's occupancy grid (copied into the env's own
 * slot before the old pool is freed) and its static rows until its next restart; the cursors are
 * set back to e mod P. */
int ebc_set_scene_pool(void *handle, const EbcScene *pool, int stride);

/* ---- SceneGenerator.generate_random_scene on the device (simulator/scene/scene_generator.py:330-378) ----
 * The keys SceneGenerator.__init__ reads (:20-72) and the per-type agent sections (agents/agent.py:16-35), with
 * the phase already resolved by the caller: count[t] / rule[t] are the number of humans of AgentType t and its
 * crossing rule for THIS phase (test_sim_* or train_val_sim_*; 1 human per type when neither `test` nor
 * multiagent_training, :343-355). */
enum EbcCrossingRule {
  EBC_RULE_CIRCLE_CROSSING = 0,     /* scene_generator.py:593-648 (adults, bicycles) */
  EBC_RULE_SQUARE_CROSSING = 1,     /* :650-712 */
  EBC_RULE_SQUARE_CROSSING_OLD = 2, /* :714-761 (bicycles only) */
  /* The crowd rules, adults only.  Each sets the number of adults itself and ignores the adult_num it is passed
   * (count[0] is not read, but for the unreachable case noted in ebc_scene_gen.h); a scene takes at most 5, 20 and 2
   * adult slots, and that capacity + count[1] + count[2] must fit max_humans. */
  EBC_RULE_MIXED = 3,               /* :523-576: 0..5 standing adults in a 4 x 8 box (p = 0.2), or 1..5 walking */
  EBC_RULE_MIXED_20 = 4,            /* :577-582, :459-501: 20 adults, randint(20) of them standing in a 6 x 8 box */
  EBC_RULE_ONE_STATIC = 5           /* :583-589: two standing adults at (-2, -8) and (-3, -8) */
};
/* adult slots a scene of each crowd rule can take */
#define EBC_CROWD_MIXED_ADULTS 5
#define EBC_CROWD_MIXED_20_ADULTS 20
#define EBC_CROWD_ONE_STATIC_ADULTS 2
#define EBC_GEN_STATIC_OVERFLOW 1 /* a generated map has more observation rows than max_static */

typedef struct EbcSceneGen {
  uint32_t struct_size;
  int32_t randomize_attributes;      /* [env] randomize_attributes */
  int32_t count[3];                  /* adults, bicycles, children */
  int32_t rule[3];                   /* EbcCrossingRule per type */
  double radius[3], v_pref[3];       /* fixed attributes ([adults] / [bicycles] / [children]) */
  double radius_min[3], radius_max[3], v_pref_min[3], v_pref_max[3]; /* sample_random_attributes, agent.py:48-56 */
  double square_width, circle_radius; /* [sim] */
  double discomfort_dist;            /* [reward] discomfort_dist (the rejection tests' margin) */
  double robot_radius, robot_v_pref; /* [robot] */
  double map_resolution, map_size_m; /* [map] */
  int32_t min_wall_length, max_wall_length, num_circles, num_walls;
} EbcSceneGen;

/* Arrays a generated batch is copied out to (ebc_generate_scenes): an EbcScene's, writable. */
typedef struct EbcSceneOut {
  uint32_t struct_size;
  int32_t location;          /* EBC_HOST or EBC_DEVICE, of every pointer below */
  int32_t *n_humans;
  double *px, *py, *vx, *vy, *gx, *gy, *radius, *v_pref;
  uint8_t *type;
  int32_t *n_static;         /* NULL allowed when max_static == 0 */
  double *spx, *spy, *sradius;
  uint64_t *grid;            /* [n][G][2] or NULL */
  double *robot;
} EbcSceneOut;

/* n scenes generated on the device, one per seed: scene i is what the reference's generate_random_scene draws after
 * np.random.seed(seeds[i]) (seeds NULL: seed0 + i; env.reset seeds with counter_offset[phase] + case,
 * simulator/env.py:153-169) — numpy's legacy MT19937 stream, draw for draw, so every value is the reference's bit
 * for bit, except the cos / sin of circle_crossing (<= 1 ulp: numpy's own results there depend on the CPU).
 * The position is circle_radius * cos: with a circle_radius that is no power of two, a cos between a power of two and
 * 4 / 3 of it lands in the next binade, and its 1 ulp is then up to 2 ulps of the position (rare: 3 of 1200 test scenes).
 * Shapes follow the handle (max_humans, max_static, grid width); sum(count) must fit max_humans (under a crowd rule
 * the rule's capacity takes the place of count[0], and n_humans then varies from scene to scene); a map with more
 * observation rows than max_static is EBC_ERR_INVALID.
 *   ebc_generate_scenes: copy the batch out (tests, inspection).
 *   ebc_generate_reset:  env.reset of envs first..first+n-1 from it, nothing crossing PCIe but the seeds.
 *   ebc_generate_pool:   install it as the EBC_FLAG_AUTO_RESET pool (as ebc_set_scene_pool, P = n). */
int ebc_generate_scenes(void *handle, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int n, EbcSceneOut *out);
int ebc_generate_reset(void *handle, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int first, int n);
int ebc_generate_pool(void *handle, const EbcSceneGen *gen, uint32_t seed0, const uint32_t *seeds, int n, int stride);

/* Humans moved by the host (BASELINE config 2): act[E][N][2]. */
int ebc_set_human_actions(void *handle, int location, const double *act);

/* EBC_HUMAN_BY_TYPE: a policy per entity type.  The reference gives [adults], [bicycles] and [children] a `policy` key
 * each (simulator/agents/agent.py:19, simulator/policy/policy_factory.py:10-14) and env.step asks every human's own
 * policy object for its action (simulator/env.py:392-405), so adults on ORCA among bicycles that ride straight on
 * `linear` is a valid scene.  policy_of_type[t], t = EBC_ADULT, EBC_BICYCLE, EBC_CHILD, is EBC_HUMAN_ORCA or
 * EBC_HUMAN_LINEAR; anything else is EBC_ERR_INVALID and ebc_last_error names the entry.  A fresh handle holds three
 * EBC_HUMAN_ORCA; the table stays until it is set again (ebc_reset and restarts do not touch it).
 *   The rule.  From the pre-step state a human of type t takes the velocity that policy_of_type[t] gives it:
 * EBC_HUMAN_ORCA the velocity EBC_HUMAN_ORCA gives that human from the same state, bit for bit (its neighbours are all
 * the others with their current velocities, humans on `linear` included, and the robot when robot_visible);
 * EBC_HUMAN_LINEAR the one EBC_HUMAN_LINEAR gives it.  The rest of the step is the step with those velocities: every
 * output and the state left behind are what EBC_HUMAN_EXTERNAL leaves when it is given exactly those [E][N][2] doubles.
 * So a table of three EBC_HUMAN_ORCA is an EBC_HUMAN_ORCA step and a table of three EBC_HUMAN_LINEAR an
 * EBC_HUMAN_LINEAR step.
 *   Every entry that takes a human_policy takes the code: ebc_step, ebc_step_with_map, ebc_lookahead (the humans are
 * evaluated once; a following EBC_HUMAN_CACHED step reads the mixed velocities), ebc_step_k and ebc_step_k_om with every
 * robot policy, and ebc_sail_dagger_k.  ebc_step is ONE launch as with EBC_HUMAN_ORCA (and what is said of that launch
 * at ebc_step holds); the groups of the humans on `linear` solve nothing.  EBC_FLAG_ONE_LAUNCH takes the code with any
 * table, bit for bit the per-step form as for every other combination: a table of three EBC_HUMAN_LINEAR is the way to
 * roll linear humans out in one launch (plain EBC_HUMAN_LINEAR stays refused there).
 *   The call waits for the handle's stream: no enqueued launch sees the table change. */
int ebc_set_human_policies(void *handle, const int32_t policy_of_type[3]);

/* The observation of the CURRENT state, without stepping: what env.reset returns
 * (simulator/env.py:188-193) and what MultiHumanRL.transform builds from it
 * (rl/policy/multi_human_rl.py:128-149).  ob [E][R][5], obs_rotated [E][R][T]; either may be NULL. */
int ebc_observe(void *handle, int location, double *ob, float *obs_rotated);

/* ORCA.predict with the ROBOT as the agent, for every env (simulator/policy/orca.py:85-157 called
 * through Robot.act, simulator/agents/robot.py:16-25): the demonstrator of the imitation-learning
 * stage (rl/train.py:99-143, which sets the policy's safety_space itself; rl/utils/explorer.py:33-45).
 * The others are the rows of the observation in their order: humans, then the static obstacles as
 * pedestrians.  action [E][2] = ActionXY; feed it to ebc_step (EBC_ROBOT_EXTERNAL).  Holonomic robots,
 * N + S <= 128 (every handle ebc_create accepts): up to 32 rows a lane per row; above, the max_neighbors nearest rows
 * in range are selected first, as Agent::insertAgentNeighbor keeps them, and the same solve runs on those. */
int ebc_robot_orca(void *handle, double safety_space, int location, double *action);

/* The demonstrator's PERSISTENT rvo2 simulator (simulator/policy/orca.py:96-133).  The reference's ORCA policy object
 * keeps one simulator for all its predict() calls and rebuilds it only when the number of agents changes
 * (orca.py:96-101); otherwise it updates positions and velocities only (:129-133), so the rows' radii
 * (+ 0.01 + safety_space), the robot's radius and its maxSpeed stay those of the call that BUILT the simulator — also
 * across env.reset(): rl/train.py:130-133 makes ONE il_policy for every imitation-learning episode, and with
 * randomize_attributes = true episodes 2... run on the radii of the episode that built it.
 * enable != 0: from now on ebc_robot_orca and EBC_ROBOT_ORCA (ebc_step_k) of this handle behave like that, one
 * simulator per env (an env = one policy object playing its episodes one after the other), all of them "not built
 * yet" (= a fresh policy object; call it again for the next one).  enable == 0 (the default): every call works from
 * the current state alone (= a fresh policy object per call).  ebc_reset and restarts do not touch the simulators. */
int ebc_robot_orca_sim(void *handle, int enable);
/* Read (set == 0) or replace (set != 0) the simulators: rows [E] (number of agents besides the robot, -1 = not built),
 * radius [E][N + S] (float, as rvo2 holds them: row j of the observation), self [E][2] = {radius, maxSpeed}.  The
 * single-env facade keeps a policy object's simulator in the object and hands it to whichever handle serves it. */
int ebc_robot_orca_sim_state(void *handle, int location, int set, int32_t *rows, float *radius, float *self);

/* One env.step for every env (simulator/env.py:388-466), enqueued on the handle's stream.  With
 * EBC_HUMAN_ORCA it is ONE kernel launch whose arguments change from call to call (the robot state
 * is double-buffered and a launch counter travels with the launch): call it once per step; do not
 * capture it in a HIP graph and replay it (a call on a stream under capture returns EBC_ERR_UNSUPPORTED and
 * records nothing).  A broken hand-off inside that launch (never seen)
 * surfaces as EBC_ERR_DEVICE — not as a hang — from ebc_synchronize or from the next host-location
 * call (whose copy-back carries the fault word); it is reported once, the handle then refuses
 * steps (EBC_ERR_STATE) until ebc_reset has re-armed it. */
int ebc_step(void *handle, const EbcStepArgs *args);
int ebc_lookahead(void *handle, const EbcLookaheadArgs *args);

/* K consecutive env.step calls for every env with a robot policy that lives on the device, in ONE call: the
 * episode loop of Explorer.run_one_episode (rl/utils/explorer.py:33-45: act -> step -> keep state, action,
 * reward) without a host round trip per step — with EBC_ROBOT_ORCA the imitation-learning rollouts of
 * rl/train.py:124-133.  Per step k the library enqueues: the rotated joint state the policy sees
 * (MultiHumanRL.transform, rl/policy/multi_human_rl.py:128-149 -> state_rotated[k]), the robot's action
 * (EBC_ROBOT_ORCA: ebc_robot_orca with robot_safety_space; EBC_ROBOT_LINEAR; EBC_ROBOT_EXTERNAL:
 * robot_action[k]), and ebc_step with every output written at index k.  Same arithmetic, launch for launch,
 * as K calls of ebc_observe / ebc_robot_orca / ebc_step (tests hold it equal to K oracle steps); what it
 * removes is the per-step host work.  EBC_FLAG_AUTO_RESET keeps every env in an episode.
 *
 * EBC_FLAG_ONE_LAUNCH: the same K steps as ONE kernel launch.  A workgroup owns a few envs for the whole call, keeps
 * their state in LDS between steps and separates the phases of a step with workgroup barriers; state is read once
 * and written once, and per step only the requested outputs, robot_action[k], the grid window and an ending env's
 * restart scene touch memory.
 *   - Same arguments, the same outputs at the same [k] indices, the same state left behind, BIT FOR BIT, as the
 *     per-step form: humans, robot, time, arrival, done, float tile, grid slot, pool cursor and the persistent
 *     simulators of ebc_robot_orca_sim hold what K per-step steps would have left, so ebc_step, ebc_lookahead,
 *     ebc_observe, ebc_get_state, ebc_local_map and a further ebc_step_k of either form continue from it.
 *   - Covers EBC_HUMAN_ORCA and EBC_HUMAN_BY_TYPE (any table, ebc_set_human_policies) with each robot policy (EBC_ROBOT_EXTERNAL reading robot_action[k], EBC_ROBOT_LINEAR,
 *     EBC_ROBOT_ORCA with or without the persistent simulator), with and without EBC_FLAG_AUTO_RESET, own-scene
 *     and installed pools, both row widths, holonomic and unicycle robots where the per-step form takes them,
 *     every output optional, host and device location.
 *   - Strict: EBC_HUMAN_LINEAR and EBC_HUMAN_EXTERNAL return EBC_ERR_UNSUPPORTED, and so does EBC_ROBOT_ORCA on a handle
 *     of more than 32 observation rows (N + S > 32: the demonstrator inside the rollout is one 32-lane group; the
 *     per-step form takes such handles); nothing else is left out (every handle ebc_create accepts fits).  The call never falls back to the per-step form.  Every refusal of ebc_step_k (capturing
 *     stream, EBC_FLAG_BORDER, K < 1, before reset, faulted handle) holds for it too.
 *   - No mailboxes, no polling, no give-up path: this launch cannot raise the handle's fault word.
 *
 * EBC_ROBOT_SAIL: the network attached with ebc_robot_sail (below) decides every step, a closed loop on the device.
 *   - Per-step form: per step k the library enqueues the gathers of the robot state, the world-frame observation rows
 *     and the row counts into scratch the handle owns (what ebc_get_state, ebc_observe and ebc_row_counts give), the
 *     kernel of ebc_sail_forward writing the action into robot_action_out[k] (or the handle's scratch when that is
 *     NULL), and ebc_step reading it: launch for launch ebc_sail_forward on the env's state followed by ebc_step.
 *   - EBC_FLAG_ONE_LAUNCH: the network runs inside the rollout kernel from the LDS-resident state, on all four waves
 *     of the workgroup before the humans' ORCA passes; outputs and state are the per-step form's bit for bit.  The
 *     network's LDS area for one env is 4 * (adult_num * (max(4 adult_num, 64) + 134) + 272) bytes (2.6 KB at
 *     adult_num 2, 4.9 KB at 5, 8.8 KB at 10, 13.4 KB at 16, 22.6 KB at 24, 33.8 KB at 32) behind the env's rollout
 *     arrays, and one env of each has to fit the kernel's 48 KB.  With R = max_humans + max_static rows of 17 floats:
 *     adult_num <= 10 fits every handle ebc_create accepts; adult_num 16 up to R = 125, 20 up to R = 98, 24 up to
 *     R = 68, 28 up to R = 34 whatever max_humans is (more rows with more humans: R = 118, 112, 76 with max_humans =
 *     adult_num); adult_num 32 only with R <= 36.  What does not fit returns EBC_ERR_UNSUPPORTED and ebc_last_error
 *     gives both sizes; the call never falls back to the per-step form.
 *   - The arrival rule ((0, 0) inside the goal radius), the NaN action of an env whose row count is not adult_num
 *     and both kinematics (the two outputs are ActionXY or ActionRot as ebc_step takes them) are ebc_sail_forward's.
 *   - Refused before anything is enqueued: no network attached (EBC_ERR_STATE), and every refusal above. */
typedef struct EbcStepKArgs {
  uint32_t struct_size;
  int32_t location;      /* of every pointer below */
  int32_t K;             /* steps, >= 1 */
  int32_t human_policy;  /* EBC_HUMAN_ORCA, _LINEAR, _BY_TYPE or _EXTERNAL (the same supplied velocities every step) */
  int32_t robot_policy;  /* EBC_ROBOT_ORCA, _LINEAR, _EXTERNAL or _SAIL */
  int32_t flags;
  double robot_safety_space;  /* EBC_ROBOT_ORCA: the policy's safety_space (rl/train.py:127-129) */
  const double *robot_action; /* [K][E][2], EBC_ROBOT_EXTERNAL only */
  /* outputs, each may be NULL */
  float *state_rotated;     /* [K][E][R][T] rotated joint state BEFORE step k (policy.last_state, explorer.py:43) */
  long long *n_rows;        /* [K][E] observation rows that exist before step k (ebc_row_counts) */
  double *robot_action_out; /* [K][E][2] the action taken at step k */
  double *reward;           /* [K][E] */
  uint8_t *done;            /* [K][E] */
  uint8_t *info;            /* [K][E] */
  double *dmin;             /* [K][E][3] */
  double *dist_to_goal;     /* [K][E] */
  float *obs_rotated;       /* [K][E][R][T] rotated observation returned by step k */
} EbcStepKArgs;
int ebc_step_k(void *handle, const EbcStepKArgs *args);
int ebc_get_state(void *handle, const EbcStateView *view);

/* Rows of the observation that exist, per env: len(ob) of the list env.step returns (humans, then the
 * static obstacles as pedestrians: simulator/env.py:381-382, :457-458) — the first dimension of the
 * state tensor MultiHumanRL.transform builds (rl/policy/multi_human_rl.py:128-149).  n_rows [E] int64
 * (what ebc_pair_mean / ebc_pair_attend take as n_valid).  Read from the device state, so it follows
 * auto-reset restarts from a scene pool whose scenes differ in size. */
int ebc_row_counts(void *handle, int location, long long *n_rows);

/* Imitation-learning value targets of a rollout window (rl/utils/explorer.py:159-170 over the episodes of
 * ebc_step_k's outputs): value[t][e] = sum over the rest of ITS episode of gamma_bar^(t' - t) reward[t'][e], walked
 * backwards per env; keep[t][e] = 1 when that episode ended inside the window in ReachGoal or a collision (the
 * reference stores whole episodes, successes and collisions only: explorer.py:82-92).  reward float64, done / info
 * uint8 [K][E] (device), values float64 [K][E], keep uint8 [K][E]; stream: hipStream_t. */
int ebc_il_targets(void *stream, const double *reward, const uint8_t *done, const uint8_t *info, int K, int E,
                   double gamma_bar, double *values, uint8_t *keep);

/* ---- get_local_map_angular on the device (simulator/env.py:468-628) ------------------------------------------
 * env.reset and env.step return (ob, local_map, ...) with compute_local_map=True by default (env.py:188-205,
 * :460-465): `dim` sector minima of the distances between the four corners of the robot's box and the obstacle
 * polygons, in the robot's heading frame, / max_range when normalize.  Same arithmetic as the reference, operation
 * for operation (csrc/ebc_local_map.h states the one place it may differ: atan2 picks sectors).
 *   ebc_local_map_config: dim ([map] angular_map_dim, <= 128, else EBC_ERR_UNSUPPORTED), max_range
 *     (angular_map_max_range), angle_min / angle_max in radians (angle_min * pi, env.py:80-84).  Allocates the
 *     polygon storage: [E + P][S][4] vertices plus a count per scene slot — the slots of the occupancy grids (an
 *     env's own ebc_reset slot, the pool's scenes).  Until this call nothing is allocated and nothing launched.
 *   ebc_set_obstacles: the polygons (scene.obstacle_vertices, scene_generator.py:109-328) of the listed envs'
 *     ebc_reset scenes (env_ids NULL = 0..n-1); ebc_set_obstacle_pool: those of the installed pool (n = its P).
 *     Every polygon is an axis-aligned 4-vertex rectangle (all the generator and saved scenes hold); anything
 *     else, or more than S polygons, is EBC_ERR_INVALID.  ebc_generate_reset / ebc_generate_pool write the
 *     polygons of the scenes they generate themselves.
 *   ebc_reset marks its envs' slots unset, ebc_set_scene_pool the pool's (ebc_generate_pool sets them): a map is
 *     EBC_ERR_STATE, naming the env or pool scene, while any slot an env can reach is unset.
 *   ebc_local_map: out [E][dim] float64, the map of the CURRENT state — what env.reset returns and what the
 *     look-ahead returns (env.py:460-465 with update=False).
 *   ebc_step_with_map: ebc_step, plus local_map [E][dim] of each env's post-step state (with EBC_FLAG_AUTO_RESET
 *     a terminal env's is that of its terminal state, like every other output of the step).  Same refusals as
 *     ebc_step; the map is worked out from the pre-step state and the step's robot action. */
typedef struct EbcLocalMapParams {
  uint32_t struct_size;
  int32_t dim;
  double max_range;
  double angle_min, angle_max;
  int32_t normalize;
  int32_t reserved;
} EbcLocalMapParams;

typedef struct EbcObstacles {
  uint32_t struct_size;
  int32_t n;
  const int32_t *n_poly;  /* [n] polygons per scene, <= S */
  const double *vertices; /* [n][S][4][2] host */
} EbcObstacles;

int ebc_local_map_config(void *handle, const EbcLocalMapParams *params);
int ebc_set_obstacles(void *handle, const int32_t *env_ids, const EbcObstacles *obstacles);
int ebc_set_obstacle_pool(void *handle, const EbcObstacles *obstacles);
int ebc_local_map(void *handle, int location, double *out);
int ebc_step_with_map(void *handle, const EbcStepArgs *args, double *local_map);

/* Geometry of the handle (E, N, S, T, G). */
int ebc_dims(void *handle, int32_t out[5]);

/* Timing aid for bench.py: average device milliseconds per ebc_step kernel
 * launch since the last call with reset != 0, measured with HIP events on the
 * stream the kernel runs on.  Enabled by ebc_timing(handle, 1). */
int ebc_timing(void *handle, int enable);
int ebc_timing_read(void *handle, int reset, double *avg_ms, int64_t *launches);

/* ---- value-network layers (the consumer of ebc_lookahead's rows) -------------------------------
 * A two-layer block of the reference's mlp() helper (rl/policy/cadrl.py:13-21: Linear + ReLU stacks;
 * rl/policy/sarl.py:25-35 builds mlp1 / mlp2 / attention / mlp3 from it):
 *     y = [relu] (W2 relu(W1 x + b1) + b2),   x [M][K0] -> y [M][O]   (float32, device)
 * on the bf16 matrix cores with every float32 operand split in two bf16 numbers (three products kept):
 * float32-grade results (tests/test_value_net.py: 4e-5 relative; 1.5e-5 on the value of the reference's
 * decision runs) at several times the float32 GEMM rate, the hidden layer never leaving the registers.
 * w1 [H][K0], b1 [H], w2 [O][H], b2 [O]: host pointers, torch.nn.Linear layout.  K0, O <= 224.
 * Optional third layer with ONE output (the attention score): w3 [O], b3 [1] (NULL = none); forward
 * then writes y [M] = w3 . relu(W2 ... + b2) + b3 and the [M][O] activations never reach memory. */
int ebc_mlp2_create(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2,
                    const float *b2, const float *w3, const float *b3, void **mlp_out);
/* x, y: device pointers; stream: hipStream_t (NULL = the null stream); relu_out: ReLU on y.
 * row_bias (device, NULL = none) [M / group_rows][H]: added to the hidden pre-activation of every row of
 * a group of group_rows consecutive rows — ValueNetwork's attention input cat([h, mean(h)]) (sarl.py:56-62)
 * without the concatenation: the mean's half of the first attention layer acts once per pair. */
int ebc_mlp2_forward(void *mlp, void *stream, const float *x, int M, int relu_out, const float *row_bias,
                     int group_rows, float *y);
int ebc_mlp2_destroy(void *mlp);

/* The per-pair glue of ValueNetwork.forward between those blocks (rl/policy/sarl.py:52-78), one pass over
 * the activations each.  A pair = one joint state = R consecutive rows, the first n_valid[b] of which exist
 * (device int64 [B]; NULL = all R).  Device pointers, 16-byte aligned; H and F multiples of 4, F <= 256.
 *   ebc_pair_mean:   g [B][H] = mean over the pair's rows of h [B*R][H]            (sarl.py:56-58)
 *   ebc_pair_attend: out [B][F] = sum_r softmax'(scores)[b][r] feat [B*R][F], softmax' = exp(s) (s != 0)
 *                    normalised over the pair's rows                                 (sarl.py:69-76) */
int ebc_pair_mean(void *stream, const float *h, const long long *n_valid, int B, int R, int H, float *g);
int ebc_pair_attend(void *stream, const float *scores, const float *feat, const long long *n_valid, int B, int R,
                    int F, float *out);

/* Activations handed from block to block already split and in fragment order (round 3).  A block created with
 * EBC_MLP_IN_FRAGMENTS takes its input as the tensor another block wrote with `frag_out`: per 32-row tile and 32-column
 * tile, the two k-steps' hi / lo bf16 fragments as the matrix cores take them (16 bytes per lane and piece; the same 4
 * bytes per element as float32 rows, rows and columns padded to 32) — the consumer's input phase is 16-byte loads,
 * no transposition through LDS and no per-lane splitting.  Both sides tile the rows from row 0 in steps of 32.
 * ebc_mlp2_forward_ex: every form of the forward in one call: x (rows) or frag_in; y (rows, may be NULL), partial /
 * seg_rows / row_weight as in ebc_mlp2_forward_reduce, frag_out [ceil(M / 32)][ceil(O / 32)][2][2][64] x 16 bytes. */
#define EBC_MLP_IN_FRAGMENTS 1
#define EBC_MLP_GENERAL_KERNEL 1
typedef struct EbcMlpArgs {
  uint32_t struct_size;
  int32_t M, relu_out, group_rows, seg_rows;
  int32_t flags; /* EBC_MLP_GENERAL_KERNEL: the general block even where a specialised kernel exists (the streamed
                    attention block of ebc_vn_stream.h takes fragment input + row_bias + a one-output third layer at
                    7 x 7 x 7 tiles): same values bit for bit — for measurements and for the test that says so */
  const float *x;
  const void *frag_in;
  const float *row_bias;
  const float *row_weight;
  float *y;
  double *partial;
  void *frag_out;
} EbcMlpArgs;
int ebc_mlp2_create_ex(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *w3, const float *b3, int flags, void **mlp_out);
int ebc_mlp2_forward_ex(void *mlp, void *stream, const EbcMlpArgs *args);

/* Refresh an existing block from weights in DEVICE memory (torch Linear layout, the shapes it was created with),
 * enqueued on `stream`: the packed split-bf16 fragments, the biases and the float32 copies are rebuilt by a kernel,
 * bit-equal to what ebc_mlp2_create packs on the host.  The training loop of rl/train.py:239-259 changes the network
 * every round; its rollouts are decisions like any others and run on the matrix-core blocks after one such call per
 * block and round.  w3 / b3: the one-output third layer, for blocks created with one (b3 is read back: one sync). */
int ebc_mlp2_update(void *mlp, void *stream, const float *w1, const float *b1, const float *w2, const float *b2,
                    const float *w3, const float *b3);

/* The same block in plain float32 on the vector ALUs (every product an fmaf into a float32 sum, like a float32 GEMM):
 * for the few rows whose value decides an argmax — SarlValueNet.action_values re-evaluates the candidates that lie
 * within the split-bf16 error of the best one (rl/policy/multi_human_rl.py:61-80 takes the maximum of float32 values).
 * Same arguments and outputs as ebc_mlp2_forward. */
int ebc_mlp2_forward_f32(void *mlp, void *stream, const float *x, int M, int relu_out, const float *row_bias,
                         int group_rows, float *y);

/* The same two reductions folded into the block that PRODUCES the activations, so that no second pass reads them
 * (and the features the attention weights multiply are never written at all):
 *   ebc_mlp2_forward_reduce: ebc_mlp2_forward, and per 32-row tile the row-weighted sums of y over each group of
 *     seg_rows (16 <= seg_rows, = R) consecutive rows the tile touches: partial [ceil(M / 32)][3][O] (device, float64).
 *     row_weight [M] (device; NULL = 1).  y NULL: the activations are not stored.  O a multiple of 4.
 *   ebc_pair_weights: w [B][R] = softmax'(scores) of ebc_pair_attend — the row weights of the feature block.
 *   ebc_pair_mask:    w [B][R] = 1 for rows < n_valid[b], else 0 — the row weights of a masked mean.
 *   ebc_pair_combine: out [B][O] = the sum of pair b's partials (two or three tiles), / n_valid[b] when mean != 0:
 *     with row weights 1 (or the mask) the pair mean of sarl.py:56-58, with ebc_pair_weights the weighted feature
 *     sum of sarl.py:73-76.  The sums are carried in float64 (float32 x float32 products are exact there) and rounded
 *     to float32 once: the result does not depend on where in the batch a pair's rows lie, and equals the one-pass
 *     kernels' to float32 rounding. */
int ebc_mlp2_forward_reduce(void *mlp, void *stream, const float *x, int M, int relu_out, const float *row_bias,
                            int group_rows, float *y, int seg_rows, const float *row_weight, double *partial);
int ebc_pair_weights(void *stream, const float *scores, const long long *n_valid, int B, int R, float *w);

/* The WIDE two-layer block: 1 <= K0, H, O <= 640 (ebc_sarl_net_create_layers' limit: the reference's policy_x3 /
 * policy_x4 networks), same arguments as ebc_mlp2_create_ex, same handle type.  Two launches of a single-layer
 * split-bf16 kernel, the hidden layer making a round trip through a scratch the handle owns (one per stream, grown on
 * demand); same arithmetic as the block above, deterministic (no atomics), not byte-equal to it.  flags: 0.
 * On its handle work: ebc_mlp2_forward (relu_out, row_bias / group_rows, the one-output tail w3 / b3),
 * ebc_mlp2_forward_f32 (the float32 matrix instruction: per output one float32 chain, k ascending), ebc_mlp2_update,
 * ebc_mlp2_destroy, and ebc_mlp2_forward_ex with plain rows (x, y, row_bias), which is ebc_mlp2_forward.
 * Refused with EBC_ERR_UNSUPPORTED, nothing written, the handle still good: EBC_MLP_IN_FRAGMENTS at creation;
 * frag_in / frag_out, partial / seg_rows / row_weight and EBC_MLP_GENERAL_KERNEL in ebc_mlp2_forward_ex;
 * ebc_mlp2_forward_reduce; and a forward on a stream under capture when the call would have to allocate the scratch
 * or raise a kernel's LDS limit (run the same call once outside the capture first). */
int ebc_mlp2_create_wide(int device_id, int K0, int H, int O, const float *w1, const float *b1, const float *w2,
                         const float *b2, const float *w3, const float *b3, int flags, void **mlp_out);

/* The argmax side of MultiHumanRL.predict for a batch (rl/policy/multi_human_rl.py:72-80), one launch:
 *   values [E][A] (float64) = reward + discount * v      (v [E][A]: the value network's float32 outputs)
 *   order  [E][A] (int32)   = each env's actions by value, best first (equal values: the lower action index first);
 *                             NaN values last, in index order: always a permutation of 0 .. A - 1
 *   count  [E]    (int32)   = how many of them lie within `bound` of the env's best non-NaN value: the prefix of `order`
 *                             that can hold the float32 network's best action when the values carry an error of
 *                             bound / 2; -1 when the values cannot rank the env (a NaN among them, or none above -inf):
 *                             every action of it is a candidate
 * Device pointers; 1 <= A <= 1024, bound >= 0.  (What ebcsim.sarl.SarlValueNet.action_values selects its re-evaluated
 * candidates from.) */
int ebc_decision_rank(void *stream, const float *v, const double *reward, double discount, double bound, int E, int A,
                      double *values, int32_t *order, int32_t *count);
/* The re-evaluated candidates back into the values, one launch: for i < n, values[env[i]][act[i]] = reward[env[i]][act[i]] +
 * discount * exact[i] (exact: the float32 network's values of the n candidates; env / act: int64 indices), and
 * *worst (float, zeroed by the caller) = max_i |exact[i] - v[env[i]][act[i]]| — the error of the matrix-core values
 * where it matters, which the caller holds against its bound.  A pair that is NaN in both forms, or the same infinity,
 * differs by 0; any other NaN difference makes *worst a NaN (above every bound).  Device pointers. */
int ebc_decision_apply(void *stream, const float *exact, const float *v, const long long *env, const long long *act,
                       const double *reward, double discount, int A, int n, double *values, float *worst);
int ebc_pair_mask(void *stream, const long long *n_valid, int B, int R, float *w);
int ebc_pair_combine(void *stream, const double *partial, const long long *n_valid, int B, int R, int O, int mean,
                     float *out);

/* ---- the LSTM of the LSTM-RL value networks (rl/policy/lstm_rl.py:9-69: nn.LSTM(input, H, batch_first), h0 = c0 = 0,
 * h_n) as one scan kernel over at most R rows per joint state, float32 (csrc/ebc_lstm_cell.h: the arithmetic, one
 * definition for the kernel and for the host build tests/native/lstm_host.cc compares it with bit for bit).
 * 1 <= I, H <= 64 and 1 <= R <= 128, else EBC_ERR_UNSUPPORTED (ebc_last_error names the one).
 *   ebc_lstm_create:  w_ih [4H][I], w_hh [4H][H], b_ih [4H], b_hh [4H]: HOST pointers, torch layout (gates i, f, g, o).
 *   ebc_lstm_update:  the same four from DEVICE memory, enqueued on `stream` (as ebc_mlp2_update): the packed weights
 *                     get the bytes a fresh ebc_lstm_create would give them.
 *   ebc_lstm_forward: sequence b runs steps t = 0 .. n_valid[b]-1 on rows b * R + t of x; n_valid[b] = 0 leaves
 *                     h_n = 0, values above R count as R (below 0 as 0).  Steps past a sequence's end keep h and c by
 *                     selection: a NaN in a padding row cannot reach the result, and a sequence's result depends on
 *                     nothing but its own rows.  h_n goes to out[b * out_stride + out_offset ..+H); with self_src the
 *                     first self_cols floats of self_src[b * self_stride ..] go to out[b * out_stride ..) — the joint
 *                     vector [self_state | h_n] of lstm_rl.py:31 without a concatenation pass (self_cols <=
 *                     out_offset, out_offset + H <= out_stride).  Nothing else of `out` is written.  A stream under
 *                     capture is refused with EBC_ERR_UNSUPPORTED. */
typedef struct EbcLstmArgs {
  uint32_t struct_size;
  int32_t B, R;
  int32_t out_offset;
  int32_t self_cols;
  int32_t reserved;
  int64_t out_stride;      /* floats between two sequences' outputs */
  int64_t self_stride;     /* floats between two sequences' self_src rows */
  const float *x;          /* device float32 [B * R][I] */
  const int64_t *n_valid;  /* device int64 [B]; NULL = all R rows */
  float *out;              /* device float32 */
  const float *self_src;   /* device float32, or NULL */
} EbcLstmArgs;
int ebc_lstm_create(int device_id, int I, int H, const float *w_ih, const float *w_hh, const float *b_ih,
                    const float *b_hh, void **lstm_out);
int ebc_lstm_update(void *lstm, void *stream, const float *w_ih, const float *w_hh, const float *b_ih,
                    const float *b_hh);
int ebc_lstm_forward(void *lstm, void *stream, const EbcLstmArgs *args);
int ebc_lstm_destroy(void *lstm);

/* ---- the decision of the CADRL policy (rl/policy/cadrl.py:194-217): the value network runs on every (robot, other)
 * row separately, an action is worth reward + discount * the MINIMUM over its rows, and the first action above every
 * earlier one is taken (csrc/ebc_cadrl_rule.h: the rule, one definition for the kernel and for the host build
 * tests/native/cadrl_host.cc compares it with byte for byte).
 *   m[e][a]      = min of v[e][a][0 .. n_valid[e]) as torch.min computes it: a NaN among those rows makes it NaN; rows at
 *                  or past n_valid[e] are never read; n_valid[e] = 0 gives NaN; values above R count as R, below 0 as 0
 *   values[e][a] = reward[e][a] + discount * (double)m[e][a], two rounded float64 operations
 *   choice[e]    = the first a whose value is greater than every earlier non-NaN value (a NaN is never chosen); -1
 *                  where no value is above -inf
 * Device pointers; 1 <= A <= 128 and 1 <= R <= 128, else EBC_ERR_UNSUPPORTED (ebc_last_error names the one).  A stream
 * under capture is refused with EBC_ERR_UNSUPPORTED. */
typedef struct EbcCadrlArgs {
  uint32_t struct_size;
  int32_t E, A, R;
  double discount;
  const float *v;          /* device float32 [E][A][R]: the network's output per row, in the sweep's row slots */
  const int64_t *n_valid;  /* device int64 [E]; NULL = all R rows */
  const double *reward;    /* device float64 [E][A] */
  double *values;          /* device float64 [E][A] */
  int32_t *choice;         /* device int32 [E] */
} EbcCadrlArgs;
int ebc_cadrl_decide(void *stream, const EbcCadrlArgs *args);

/* ---- the occupancy maps of OM-SARL (rl/policy/multi_human_rl.py:156-227 build_occupancy_maps; :62-69 appends them to
 * the rotated rows of every candidate action; :151-154 input_dim = T + cell_num^2 * om_channel_size).  The arithmetic is
 * csrc/ebc_om_rule.h, one definition for the kernel and for the host build tests/native/om_host.cc compares it with
 * byte for byte; it states the reference's arctan2 / cos / sin frame algebraically.
 *   For every row a < n_valid[e] of next_ob[e] (px, py, vx, vy, radius: the look-ahead's next_ob as it stands) and
 *   every OTHER row o < n_valid[e] (by index: two rows at the same place still see each other, :177): o's position in
 *   the frame whose x axis is a's velocity, binned by floor(coord / cell_size + cell_num / 2) per axis (:192-198),
 *   dropped outside [0, cell_num).  W = cell_num^2 * channels floats per row: channels 1 = occupied 0 / 1 (:199-201),
 *   2 = the mean velocity of the cell's occupants in a's frame, 3 = (1, mean vx, mean vy) (:203-225); empty cells are 0;
 *   float64 sums in row order, one cast to float32 (:227).
 *   om[e][r][W]            the maps; rows at or past n_valid[e] are never read (a NaN there reaches nothing) and get 0
 *   rows_wide[e][a][r][T + W] = rows[e][a][r][0 .. T) | om[e][r]: the maps are built once per env, from the state
 *                          every action shares (:63-66), and appended to every action's rows
 * Device pointers.  Either output may be NULL, not both; rows_wide needs rows.  No atomics: a result does not depend
 * on the launch shape.  EBC_ERR_UNSUPPORTED (ebc_last_error names the one) for channels outside {1, 2, 3}, cell_num < 1,
 * cell_size not a finite positive number, W > 192, R > 128 and, with rows_wide, A > 128 or T + W > 224 (the input limit
 * of the two-layer blocks); a stream under capture is refused with EBC_ERR_UNSUPPORTED. */
typedef struct EbcOmArgs {
  uint32_t struct_size;
  int32_t E, A, R, T;
  int32_t cell_num;        /* [om] cell_num */
  int32_t channels;        /* [om] om_channel_size */
  int32_t reserved;
  double cell_size;        /* [om] cell_size */
  const double *next_ob;   /* device float64 [E][R][5] */
  const int64_t *n_valid;  /* device int64 [E]; NULL = all R rows; above R counts as R, below 0 as 0 */
  const float *rows;       /* device float32 [E][A][R][T], or NULL */
  float *om;               /* device float32 [E][R][W], or NULL */
  float *rows_wide;        /* device float32 [E][A][R][T + W], or NULL */
} EbcOmArgs;
int ebc_occupancy_rows(int device_id, void *stream, const EbcOmArgs *args);

/* ---- the state OM-SARL stores for training (rl/policy/multi_human_rl.py:128-149 transform = [rotate(state) |
 * build_occupancy_maps(state.agent_states)], in imitation learning and in RL alike): the env's CURRENT state, read once,
 * as one kernel (csrc/ebc_om_state.h; a workgroup per env).  In bytes:
 *   state_wide[e][r][0 .. T)     = ebc_observe's obs_rotated (zeros for rows that do not exist)
 *   state_wide[e][r][T .. T + W) = ebc_occupancy_rows' om on ebc_observe's ob with ebc_row_counts' counts (0 for rows
 *                                  that do not exist)
 *   n_rows[e]                    = ebc_row_counts (may be NULL)
 * Device pointers.  The spec has ebc_occupancy_rows' limits and its refusals by name (channels outside {1, 2, 3},
 * cell_num < 1, cell_size not a finite positive number, W > 192, R > 128, T + W > 224: EBC_ERR_UNSUPPORTED); a stream
 * under capture is refused with EBC_ERR_UNSUPPORTED; before ebc_reset and on a faulted handle EBC_ERR_STATE. */
typedef struct EbcOmSpec {
  uint32_t struct_size;
  int32_t cell_num;        /* [om] cell_num */
  int32_t channels;        /* [om] om_channel_size */
  int32_t reserved;
  double cell_size;        /* [om] cell_size */
} EbcOmSpec;
/* state_wide: device float32 [E][R][T + W]; n_rows: device int64 [E], or NULL */
int ebc_observe_wide(void *handle, const EbcOmSpec *spec, float *state_wide, long long *n_rows);

/* ---- the state OM-LSTM stores in RL (rl/policy/lstm_rl.py:117-123: LstmRL.predict sorts state.agent_states by decreasing
 * distance to the robot, then transform(state) builds the maps from the SORTED list): ebc_observe_wide with the env's
 * existing rows in that order, as one kernel (csrc/ebc_om_state.h).  The order: the rows r < n_rows[e] in a stable
 * descending order of their own rotated float32 column 11 (`da`), a NaN behind every number, several NaNs in the env's
 * order; slots past the rows stay where they are, zero rows and zero maps.  A cell's sums run over its occupants in the
 * sorted order, so this is no permutation of ebc_observe_wide's rows.  In bytes: permute ebc_observe's ob and obs_rotated
 * by that order; then
 *   state_wide[e][i][0 .. T)     = the permuted obs_rotated
 *   state_wide[e][i][T .. T + W) = ebc_occupancy_rows' om on the permuted ob with ebc_row_counts' counts
 *   n_rows[e]                    = ebc_row_counts (may be NULL)
 * Limits, refusals and states are ebc_observe_wide's. */
int ebc_observe_wide_sorted(void *handle, const EbcOmSpec *spec, float *state_wide, long long *n_rows);

/* ebc_step_k(handle, args) in its per-step form — the same outputs at the same [k], the same launches — and before
 * step k also the wide state of the state the policy sees: one enqueue of ebc_observe_wide's kernel per step, no host
 * work between steps.  What an imitation window (EBC_ROBOT_ORCA) needs to fill OM-SARL's replay.  EBC_FLAG_ONE_LAUNCH is
 * EBC_ERR_UNSUPPORTED (the window with maps has the per-step form only, the choice ebc_sail_dagger_k made);
 * state_wide is a device pointer whatever args->location says. */
typedef struct EbcStepKOm {
  uint32_t struct_size;
  int32_t reserved;
  EbcOmSpec spec;
  float *state_wide;       /* device float32 [K][E][R][T + W] */
} EbcStepKOm;
int ebc_step_k_om(void *handle, const EbcStepKArgs *args, const EbcStepKOm *om);

/* ebc_step_k(handle, args) in either form — every output of `args` and the state left behind are its bytes — and
 * before step k also the world itself, what the reference keeps per step in env.states (simulator/env.py:344-351):
 * the robot's FullState and the world-frame observation rows.  Index k is the state BEFORE step k, the convention of
 * state_rotated[k] and n_rows[k]: robot[k] holds the bytes ebc_get_state's `robot` would give there and ob[k] those of
 * ebc_observe's `ob` (rows past an env's own are zeros); after a terminal step under EBC_FLAG_AUTO_RESET index k + 1
 * shows the restart scene.  The pointers live where args->location says; at least one is non-NULL.
 *   - Per-step form: one copy of the robot array per step, and ebc_observe's kernel writing `ob` (in the launch that
 *     writes state_rotated[k] where that is asked for too).
 *   - EBC_FLAG_ONE_LAUNCH: the workgroup writes its envs' records from the LDS-resident state at the top of every step
 *     (instantiations of their own, csrc/ebcsim_world.hip; the kernels of plain ebc_step_k are not touched).
 *   - Every refusal of ebc_step_k holds; a wrong struct_size, a non-zero `reserved` or two NULL pointers are
 *     EBC_ERR_INVALID. */
typedef struct EbcStepKWorld {
  uint32_t struct_size;
  int32_t reserved;   /* 0 */
  double *robot;      /* [K][E][9]    the robot's FullState BEFORE step k (ebc_get_state's `robot`), or NULL */
  double *ob;         /* [K][E][R][5] world-frame rows BEFORE step k (ebc_observe's `ob`), or NULL */
} EbcStepKWorld;
int ebc_step_k_world(void *handle, const EbcStepKArgs *args, const EbcStepKWorld *world);

/* ---- the SAIL policy (rl/policy/sail.py): one small network from the robot's state and the world-frame states of
 * exactly adult_num others straight to a continuous action, no look-ahead and no action space; one kernel per batch of
 * decisions.  The arithmetic is csrc/ebc_sail_rule.h (one definition for the kernel and for the host build
 * tests/native/sail_host.cc compares it with byte for byte): float32, every Linear a serial fmaf chain in ascending k
 * from the bias, ReLU and the softmax's maximum by selection, exp without libm, sums ascending.
 *
 * EbcSailWeights: the 14 Linear layers of ExtendedNetwork (sail.py:15-60) in this order —
 *   0 robot_encoder.0 [32][4]    1 robot_encoder.2 [32][32]   2 adult_encoder.0 [64][4 adult_num]   3 adult_encoder.2 [64][64]
 *   4 adult_head.0 [32][64]      5 joint_embedding.0 [64][64] 6 pairwise.0 [64][64]    7 pairwise.2 [64][64]
 *   8 attention.0 [64][64]       9 attention.2 [1][64]        10 task_encoder.0 [64][4] 11 task_encoder.2 [64][64]
 *   12 joint_encoder.0 [64][128] 13 planner [2][64]
 * — HOST pointers, torch's layout [out][in], widths the reference's fixed ones (local 32, embedding 64, hidden 64:
 * SAIL.configure, sail.py:109-112, builds nothing else).  2 <= adult_num <= 32, else EBC_ERR_UNSUPPORTED and
 * ebc_last_error names what was refused (at adult_num = 1 the reference's own reshape of an empty selection raises,
 * rl/utils/transform.py:16-18).  ebc_sail_create (sail.py:109-112, the model) re-packs them for the kernel. */
#define EBC_SAIL_LAYERS 14
typedef struct EbcSailWeights {
  uint32_t struct_size;
  int32_t adult_num;                      /* [sail] adult_num */
  const float *weight[EBC_SAIL_LAYERS];   /* host float32 [out][in] */
  const float *bias[EBC_SAIL_LAYERS];     /* host float32 [out] */
} EbcSailWeights;
/* One ebc_sail_forward: SAIL.predict for E envs (sail.py:114-132 with transform :134-156, ExtendedNetwork.forward
 * :62-101, transform_frame rl/utils/transform.py:11-20, reach_destination simulator/policy/policy.py:44-52).
 *   rows at or past adult_num of an env are never read (a NaN there reaches nothing)
 *   n_rows[e] != adult_num: action NaN, feat_joint zeros (the reference raises there)
 *   an arrived env (float64 sqrt(dy*dy + dx*dx) < radius): action (0, 0); its feat_joint is still the network's
 * An env's result depends on nothing but its own inputs.  Device pointers.  A stream under capture is refused with
 * EBC_ERR_UNSUPPORTED. */
typedef struct EbcSailArgs {
  uint32_t struct_size;
  int32_t E;
  int32_t R;               /* row stride of ob, R >= adult_num */
  int32_t reserved;
  const double *robot;     /* device float64 [E][9] FullState order */
  const double *ob;        /* device float64 [E][R][5] */
  const int64_t *n_rows;   /* device int64 [E]; NULL = every env has adult_num rows */
  double *action;          /* device float64 [E][2] */
  float *feat_joint;       /* device float32 [E][64], or NULL */
} EbcSailArgs;
int ebc_sail_create(const EbcSailWeights *weights, int device_id, void **sail_out);
/* SAIL.predict for a batch (sail.py:114-132): one launch on `stream` */
int ebc_sail_forward(void *sail, void *stream, const EbcSailArgs *args);
/* frees what ebc_sail_create (sail.py:109-112) made */
int ebc_sail_destroy(void *sail);
/* Attach a network made by ebc_sail_create to an env handle as its EBC_ROBOT_SAIL policy (ebc_step_k); sail = NULL
 * detaches.  The env handle keeps the network's device weights and adult_num, not the network: DETACH (or destroy the
 * env handle) BEFORE ebc_sail_destroy.  EBC_ERR_INVALID, with the attachment as it was: the network is on another device
 * than the env handle; the env handle has max_humans + max_static < adult_num rows. */
int ebc_robot_sail(void *handle, void *sail);

/* ---- training the SAIL network by imitation: the gradient of the regression loss on a demonstrator's action with
 * respect to every weight, in one launch that runs the forward with every activation kept on chip and then the backward,
 * and a second small launch that adds the partial sums.  The arithmetic is csrc/ebc_sail_grad_rule.h (one definition for
 * the kernel and for the host build tests/native/sail_grad_host.cc compares it with byte for byte).
 *   w_e = 0 for an env that has arrived, whose n_rows is not adult_num, or whose sample_mask is 0; such an env enters no
 *     sum (a selection, never a product with 0: its NaNs reach nothing but its own `action`)
 *   loss_sum = the sum over envs of w_e * ((planned[0] - (float)target[0])^2 + (planned[1] - (float)target[1])^2)
 *   grad     = d/dweights of grad_scale / 2 * loss_sum (the seed is grad_scale * (planned - target)): grad_scale =
 *              1 / count is the mean squared error over 2 * count elements, torch's MSELoss
 *   count    = the sum of w_e
 *   action   = what ebc_sail_forward gives on the same inputs, byte for byte (NULL: not written)
 * The batch is cut into chunks of 16 consecutive envs; a weight's float32 sum runs over a chunk's envs (and their rows)
 * ascending, the chunks are added ascending in float64 and rounded once: the result depends on the inputs alone, never
 * on the grid or on timing.  grad has the layout of the packed image (ebc_sail_packed_floats floats: the 14 layers in
 * the order of EbcSailWeights, each as W[k][64] — unit u of input k at k * 64 + u — followed by bias[64]; entries past
 * a layer's width are exactly 0).  Scratch for the partial sums belongs to the network and grows on demand (growing
 * waits for the device).  Device pointers.  A stream under capture is refused with EBC_ERR_UNSUPPORTED. */
typedef struct EbcSailGradArgs {
  uint32_t struct_size;
  int32_t E;
  int32_t R;                    /* row stride of ob, R >= adult_num */
  float grad_scale;
  const double *robot;          /* device float64 [E][9] FullState order */
  const double *ob;             /* device float64 [E][R][5] */
  const int64_t *n_rows;        /* device int64 [E]; NULL = every env has adult_num rows */
  const double *target;         /* device float64 [E][2]: the demonstrator's action */
  const uint8_t *sample_mask;   /* device uint8 [E]; NULL = every env counts */
  float *grad;                  /* device float32 [ebc_sail_packed_floats] */
  double *loss_sum;             /* device float64 [1] */
  int64_t *count;               /* device int64 [1] */
  double *action;               /* device float64 [E][2], or NULL */
} EbcSailGradArgs;
int ebc_sail_grad(void *sail, void *stream, const EbcSailGradArgs *args);
/* floats of the network's packed image */
int ebc_sail_packed_floats(void *sail, int64_t *floats_out);
/* the packed image into dst_dev (device float32 [ebc_sail_packed_floats]): a copy enqueued on `stream` */
int ebc_sail_get_packed(void *sail, void *stream, float *dst_dev);
/* src_dev (device float32, the packed layout, pad entries 0) becomes the network's weights: a stream-ordered copy into
 * the network's own image, enqueued on `stream`.  Everything enqueued after it on that stream (or ordered after it)
 * computes with the new weights, also an env handle the network is attached to (ebc_robot_sail keeps a pointer to the
 * image, not a copy): its next enqueued ebc_step_k decides with them.  Work on other streams is not ordered with it. */
int ebc_sail_set_packed(void *sail, void *stream, const float *src_dev);


/* ---- DAgger for the SAIL network (Ross, Gordon and Bagnell 2011): K closed-loop steps in which the attached network
 * (ebc_robot_sail) drives while the ORCA robot of ebc_robot_orca labels every state the network visits, recorded as the
 * dataset ebc_sail_grad trains on.  Device pointers only; everything is enqueued on the handle's stream.  Per step k:
 *   1. robot[k], ob[k], n_rows[k] receive the bytes ebc_get_state (robot), ebc_observe (ob: the static rows too, zeros
 *      for rows that do not exist) and ebc_row_counts give on the current state;
 *   2. expert_action[k] receives the bytes of ebc_robot_orca(handle, expert_safety_space, ...) on that state; the
 *      persistent simulators of ebc_robot_orca_sim are left as one ebc_robot_orca call per step leaves them;
 *   3. learner_action[k] receives the bytes of ebc_sail_forward reading robot[k], ob[k], n_rows[k] in place (its arrival
 *      rule and its NaN action for a row count other than adult_num unchanged);
 *   4. robot_action_out[k][e] = take_expert[k][e] ? expert_action[k][e] : learner_action[k][e], chosen as bits, never
 *      arithmetic: a NaN of the side not taken reaches nothing;
 *   5. ebc_step takes that action with `flags` and writes the optional outputs at index k.
 * Steps 1 and 2 are one kernel that reads the state once; a step is four launches (label, network, select, step).
 * Refused before anything is enqueued, nothing written, the state untouched: no network attached (EBC_ERR_STATE); a
 * unicycle robot or max_humans + max_static > 32 (EBC_ERR_UNSUPPORTED, as ebc_robot_orca); EBC_FLAG_ONE_LAUNCH or
 * EBC_FLAG_BORDER (EBC_ERR_UNSUPPORTED: the labelled rollout has the per-step form only); a stream under capture
 * (EBC_ERR_UNSUPPORTED); K < 1, a NULL required output, a wrong struct_size, a negative or NaN safety space
 * (EBC_ERR_INVALID); before ebc_reset or on a faulted handle as ebc_step_k (EBC_ERR_STATE). */
typedef struct EbcSailDaggerArgs {
  uint32_t struct_size;
  int32_t K;                     /* steps, >= 1 */
  int32_t human_policy;          /* as ebc_step_k */
  int32_t flags;                 /* EBC_FLAG_AUTO_RESET or 0 */
  double expert_safety_space;    /* the ORCA robot's safety_space, >= 0 */
  const uint8_t *take_expert;    /* device [K][E], or NULL = the learner always acts;
                                    != 0: step k of env e executes the expert's action */
  /* required outputs, device pointers */
  double *robot;                 /* [K][E][9]    FullState before step k (ebc_get_state's robot) */
  double *ob;                    /* [K][E][R][5] world-frame rows before step k (ebc_observe's ob) */
  long long *n_rows;             /* [K][E]       (ebc_row_counts) */
  double *learner_action;        /* [K][E][2]    ebc_sail_forward on robot[k], ob[k], n_rows[k] */
  double *expert_action;         /* [K][E][2]    ebc_robot_orca on the same state */
  double *robot_action_out;      /* [K][E][2]    the action the step took */
  /* optional outputs */
  double *reward; uint8_t *done; uint8_t *info;   /* [K][E] each, or NULL */
} EbcSailDaggerArgs;
int ebc_sail_dagger_k(void *handle, const EbcSailDaggerArgs *args);

/* ---- training the CADRL value network (rl/policy/cadrl.py:13-31: four Linear layers ending in one output, ReLU after
 * the first three; rl/utils/trainer.py:74-100: MSE regression on value targets): the gradient of the loss with respect
 * to every weight, in one launch that runs the forward of every row, takes each state's minimum over its rows and runs
 * the backward through the minimal row, and a second small launch that adds the partial sums.  The arithmetic is
 * csrc/ebc_cadrl_grad_rule.h (one definition for the kernel and for the host build tests/native/cadrl_grad_host.cc
 * compares it with byte for byte): float32, every unit a serial fmaf chain over its inputs ascending from 0, then + bias.
 * Those are the forward's bytes for THIS entry; ebc_mlp2_forward_f32 (what ebc_cadrl_decide's values come from) agrees
 * with them to float32 rounding, not bit for bit.
 *
 * EbcCadrlNetWeights: n_layers = 4; widths = the row width, then the four layers' units; weight / bias: HOST pointers,
 * torch's layout [out][in] / [out].  Limits: 1 <= widths[0] <= 64, 1 <= widths[1 .. 3] <= 256, widths[4] = 1, else
 * EBC_ERR_UNSUPPORTED and ebc_last_error names the limit.
 * The packed image (weights, and the gradient alike): the four layers in order, layer l as W[k][Op] — unit u of input k
 * at k * Op + u, Op = the layer's units padded to a multiple of 4 — followed by bias[Op]; pad entries are exactly 0.
 * 27 732 floats (108 KB) at the reference's 13 -> 150 -> 100 -> 100 -> 1. */
#define EBC_CADRL_NET_LAYERS 4
typedef struct EbcCadrlNetWeights {
  uint32_t struct_size;
  int32_t n_layers;                            /* 4 */
  int32_t widths[EBC_CADRL_NET_LAYERS + 1];    /* row width, then the layers' units */
  int32_t reserved;
  const float *weight[EBC_CADRL_NET_LAYERS];   /* host float32 [out][in] */
  const float *bias[EBC_CADRL_NET_LAYERS];     /* host float32 [out] */
} EbcCadrlNetWeights;
/* One ebc_cadrl_grad over B states of R row slots each:
 *   n        = n_valid[b] clamped to [0, R] (NULL: R); rows at or past n are never read
 *   value[b] = the minimum over rows [0, n) of the network's output, as ebc_cadrl_decide takes it (a NaN among them makes
 *              it NaN, no row gives NaN); min_row[b] = the first row that holds it, -1 without rows
 *   live     = (sample_mask == NULL or sample_mask[b] != 0) and n >= 1; a state that is not live enters no sum (a
 *              selection, never a product with 0: its NaNs reach nothing but its own value); a NaN inside a live state
 *              reaches loss_sum and grad
 *   loss_sum = the sum over live states of (value - target)^2, the difference in float32, squared and summed in float64
 *   grad     = d/dweights of grad_scale / 2 * loss_sum, through each state's min_row alone (the seed is grad_scale *
 *              (value - target)): grad_scale = 2 / count is torch's MSELoss over count values
 *   count    = the number of live states
 * The batch is cut into chunks of 16 consecutive states; a weight's float32 sum runs over a chunk's live states ascending,
 * the chunks are added ascending in float64 and rounded once: the result depends on the inputs alone, never on the grid or
 * on timing.  Every NaN written is the quiet NaN 0x7fc00000 (float64: 0x7ff8000000000000).  grad has the packed layout.
 * Scratch for the partial sums belongs to the network and grows on demand (growing waits for the WHOLE device and frees
 * the old scratch).  So at most ONE ebc_cadrl_grad may be in flight per network: calls on one network go to one stream, or
 * are ordered by the caller, and never come from two threads at once; nothing locks the scratch.  A call that has to grow
 * the scratch must not be made while another stream of the process is being captured (the wait would break that capture):
 * make the first call at the largest B before capturing elsewhere.  Two networks are independent.  Device
 * pointers.  1 <= R <= 128, else EBC_ERR_UNSUPPORTED; T other than the network's row width is EBC_ERR_INVALID; a stream
 * under capture is refused with EBC_ERR_UNSUPPORTED. */
typedef struct EbcCadrlGradArgs {
  uint32_t struct_size;
  int32_t B, R, T;
  float grad_scale;
  int32_t reserved;
  const float *rows;            /* device float32 [B][R][T] */
  const int64_t *n_valid;       /* device int64 [B]; NULL = all R rows */
  const float *target;          /* device float32 [B] */
  const uint8_t *sample_mask;   /* device uint8 [B]; NULL = every state counts */
  float *grad;                  /* device float32 [ebc_cadrl_net_packed_floats] */
  double *loss_sum;             /* device float64 [1] */
  int64_t *count;               /* device int64 [1] */
  float *value;                 /* device float32 [B], or NULL */
  int32_t *min_row;             /* device int32 [B], or NULL */
} EbcCadrlGradArgs;
int ebc_cadrl_net_create(const EbcCadrlNetWeights *weights, int device_id, void **net_out);
int ebc_cadrl_net_destroy(void *net);
/* floats of the network's packed image */
int ebc_cadrl_net_packed_floats(void *net, int64_t *floats_out);
/* the packed image into dst_dev (device float32 [ebc_cadrl_net_packed_floats]): a copy enqueued on `stream` */
int ebc_cadrl_net_get_packed(void *net, void *stream, float *dst_dev);
/* src_dev (device float32, the packed layout, pad entries 0) becomes the network's weights: a stream-ordered copy,
 * enqueued on `stream`; an ebc_cadrl_grad enqueued after it on that stream computes with the new weights. */
int ebc_cadrl_net_set_packed(void *net, void *stream, const float *src_dev);
int ebc_cadrl_grad(void *net, void *stream, const EbcCadrlGradArgs *args);

/* ---- training the SARL value network (rl/policy/sarl.py:38-82; rl/utils/trainer.py:74-100: MSE regression on value
 * targets): the gradient of the loss with respect to every weight, in one launch per run of chunks that runs the forward
 * of every row of a chunk's states (mlp1, mlp2, the mean, attention, the reference's masked softmax, the weighted sum,
 * mlp3) with every activation kept in LDS and the backward through all of it, and a second small launch that adds the
 * partial sums.  The arithmetic is csrc/ebc_sarl_grad_rule.h (one definition for the kernel and for the host build
 * tests/native/sarl_grad_host.cc compares it with byte for byte).  Those are the forward's bytes for THIS entry; the
 * deciding blocks (ebc_mlp2_*) agree with them to float32 rounding, not bit for bit.
 *
 * EbcSarlNetWeights: n_mlp1 / n_mlp2 / n_attention / n_mlp3 = 2 / 2 / 3 / 4 Linear layers (anything else is
 * EBC_ERR_UNSUPPORTED); widths = the layers' units in the order mlp1, mlp2, attention, mlp3; weight / bias: HOST pointers
 * in that order, torch's layout [out][in] / [out].  Limits: 1 <= input_dim <= 64, every width 1 .. 256, the last layers of
 * attention and mlp3 one unit, 0 <= self_state_dim <= input_dim, else EBC_ERR_UNSUPPORTED and ebc_last_error names the limit.
 * The packed image (weights, and the gradient alike): the eleven layers in that order, layer l as W[k][Op] — unit u of
 * input k at k * Op + u, Op = the layer's units padded to a multiple of 4 — followed by bias[Op]; pad entries are exactly
 * 0.  97 452 floats (381 KB) at the reference's widths with the global state. */
#define EBC_SARL_NET_MAX_LAYERS 16
typedef struct EbcSarlNetWeights {
  uint32_t struct_size;
  int32_t n_mlp1, n_mlp2, n_attention, n_mlp3;   /* 2, 2, 3, 4 */
  int32_t with_global_state;
  int32_t self_state_dim;
  int32_t input_dim;                             /* the row width T */
  int32_t widths[EBC_SARL_NET_MAX_LAYERS];       /* the layers' units */
  const float *weight[EBC_SARL_NET_MAX_LAYERS];  /* host float32 [out][in] */
  const float *bias[EBC_SARL_NET_MAX_LAYERS];    /* host float32 [out] */
} EbcSarlNetWeights;
/* One ebc_sarl_grad over B states of R row slots each:
 *   n            = n_valid[b] clamped to [0, R] (NULL: R); rows at or past n are never read and receive nothing
 *   value[b]     = the network's output on the state's rows [0, n); NaN without rows
 *   attention[b] = the softmax weights of the rows [0, n) (e = exp(s) * (s != 0), no maximum subtracted), 0 at or past n
 *   live         = (sample_mask == NULL or sample_mask[b] != 0) and n >= 1; a state that is not live enters no sum (a
 *                  selection: its NaNs reach nothing but its own value and attention); a NaN inside a live state reaches
 *                  loss_sum and grad
 *   loss_sum     = the sum over the live states of (value - target)^2, count = their number
 *   grad         = d/dweights of grad_scale / 2 * loss_sum (grad_scale = 2 / count: torch's MSELoss), packed layout
 * The batch is cut into chunks of 4 consecutive states; inside a chunk a weight's sum is a float32 fmaf chain over the
 * live states and their rows ascending, the chunks are added ascending in float64 and rounded once: the result depends on
 * the inputs alone.  Every NaN written is the quiet NaN 0x7fc00000 (float64: 0x7ff8000000000000).  Scratch belongs to
 * the network and grows on demand, exactly as ebc_cadrl_grad's: at most ONE ebc_sarl_grad in flight per network.  Device
 * pointers.  1 <= R <= ebc_sarl_net_grad_max_rows (a chunk's activations must fit a workgroup's 160 KB of LDS: 15 at the
 * reference widths), else EBC_ERR_UNSUPPORTED with nothing written; T other than the network's row width is
 * EBC_ERR_INVALID; a stream under capture is refused with EBC_ERR_UNSUPPORTED.
 * states_per_pass = S: 0 is the call above.  4, 2 or 1 runs a chunk's states S at a time, so that only S states' activations
 * must fit the LDS: 1 <= R <= ebc_sarl_net_grad_max_rows_at(S) (15, 32 and 64 at the reference widths), else
 * EBC_ERR_UNSUPPORTED with nothing written and a message that names R, S and that limit.  From the second pass on, the
 * thread that owns a weight's entry continues its fmaf chain from the chunk's partial sum: the chunks, the chains and so
 * every byte written are those of states_per_pass = 0, whatever S.  Any other value is EBC_ERR_INVALID. */
typedef struct EbcSarlGradArgs {
  uint32_t struct_size;
  int32_t B, R, T;
  float grad_scale;
  int32_t states_per_pass;      /* 0 = the whole chunk at once; 4, 2, 1 = that many states of a chunk at a time */
  const float *rows;            /* device float32 [B][R][T] */
  const int64_t *n_valid;       /* device int64 [B]; NULL = all R rows */
  const float *target;          /* device float32 [B] */
  const uint8_t *sample_mask;   /* device uint8 [B]; NULL = every state counts */
  float *grad;                  /* device float32 [ebc_sarl_net_packed_floats] */
  double *loss_sum;             /* device float64 [1] */
  int64_t *count;               /* device int64 [1] */
  float *value;                 /* device float32 [B], or NULL */
  float *attention;             /* device float32 [B][R], or NULL */
} EbcSarlGradArgs;
int ebc_sarl_net_create(const EbcSarlNetWeights *weights, int device_id, void **net_out);
/* The network of OM-SARL (multi_human_rl.py:151-154: input_dim = T + cell_num^2 * om_channel_size): input_dim stays the
 * rotated width T (1 .. 64, self_state_dim <= T), om_width = W is 0 .. 192 and T + W <= 224, else EBC_ERR_UNSUPPORTED by
 * name.  mlp1's first layer has T + W inputs (weight[0] is [out][T + W]); the packed image follows the rule above with
 * that K; ebc_sarl_grad on such a network takes args.T == T + W and ebc_sarl_net_grad_max_rows answers for the wide row.
 * om_width = 0 is ebc_sarl_net_create: the same network, packed image and bytes. */
int ebc_sarl_net_create_om(const EbcSarlNetWeights *weights, int om_width, int device_id, void **net_out);
/* The LAYER form of the same gradient (csrc/ebc_sarl_grad_layers.h), for the networks the chunk form does not hold: every
 * hidden width 1 .. 640 (the reference's policy_x2 / x3 / x4 configs: 300, 400, 600); the rows' limits are those of
 * ebc_sarl_net_create_om (input_dim 1 .. 64, om_width 0 .. 192, T + W <= 224), refusals by name as there.  The packed image
 * is the same, and ebc_sarl_net_packed_floats / _get_packed / _set_packed / _destroy work on the object unchanged, so a
 * flat weight tensor passes between the two forms' networks.  ebc_sarl_grad on such a network takes the same
 * EbcSarlGradArgs and writes the same outputs, and the SAME BYTES as the chunk form where both take the network: it runs
 * the rule layer by layer over runs of whole chunks (at most 65 536 row slots a run) on the float32 matrix instruction,
 * which is a k-ordered fmaf chain per output, with every activation and delta in the network's scratch in device memory
 * (about 0.45 GB at the x2 widths, 0.9 GB at x4, for a full run); a weight's chunks are added ascending in float64 by the one
 * wave that owns it, across runs too.  Rows at or past n ARE read here, and enter nothing.  1 <= R <= 128
 * (ebc_sarl_net_grad_max_rows), else EBC_ERR_UNSUPPORTED with nothing written.  states_per_pass must be 0: 4, 2 and 1 are
 * EBC_ERR_UNSUPPORTED ("the layer form has no passes"), here and in ebc_sarl_net_grad_max_rows_at; any other value is
 * EBC_ERR_INVALID.  About 45 short launches per run. */
int ebc_sarl_net_create_layers(const EbcSarlNetWeights *weights, int om_width, int device_id, void **net_out);
int ebc_sarl_net_destroy(void *net);
int ebc_sarl_net_packed_floats(void *net, int64_t *floats_out);
int ebc_sarl_net_get_packed(void *net, void *stream, float *dst_dev);
int ebc_sarl_net_set_packed(void *net, void *stream, const float *src_dev);
/* the largest R ebc_sarl_grad takes for this network with the whole chunk at once (states_per_pass = 0) */
int ebc_sarl_net_grad_max_rows(void *net, int *rows_out);
/* the same for a value of EbcSarlGradArgs.states_per_pass: 0, 4, 2 or 1 (anything else is EBC_ERR_INVALID) */
int ebc_sarl_net_grad_max_rows_at(void *net, int states_per_pass, int *rows_out);
int ebc_sarl_grad(void *net, void *stream, const EbcSarlGradArgs *args);

/* ---- training the LSTM-RL value networks (rl/policy/lstm_rl.py:9-69: ValueNetwork1, rows -> LSTM -> mlp on cat(self
 * state, h_n), lstm_rl.py:9-32; ValueNetwork2, rows -> mlp1 -> LSTM -> mlp, lstm_rl.py:35-69; rl/utils/trainer.py:74-100: MSE
 * regression on value targets): the gradient of the loss with respect to every weight, in one launch per run of chunks
 * that runs mlp1 over every row of a chunk's states, the recurrence a step at a time, mlp, and the backward through all of
 * it, through time included, with every activation and every step's gates kept in LDS, and a second small launch that adds
 * the partial sums.  The arithmetic is csrc/ebc_lstm_grad_rule.h (one definition for the kernel and for the host build
 * tests/native/lstm_grad_host.cc compares it with byte for byte); the recurrence's forward is csrc/ebc_lstm_cell.h's, so
 * ValueNetwork1's h_n is ebc_lstm_forward's, bit for bit.
 *
 * EbcLstmNetWeights: n_mlp1 = 0 (ValueNetwork1) or 4, n_mlp = 4 Linear layers (anything else is EBC_ERR_UNSUPPORTED);
 * widths / weight / bias [0 .. 3]: mlp1's layers (not read when n_mlp1 = 0), [4 .. 7]: mlp's; HOST pointers, torch's layout
 * [out][in] / [out]; w_ih [4 H][I], w_hh [4 H][H], b_ih [4 H], b_hh [4 H] as nn.LSTM keeps them (gate order i, f, g, o).
 * Limits: 1 <= input_dim <= 64, the LSTM's input and hidden_dim 1 .. 64, every Linear width 1 .. 256, the last layer of mlp
 * one unit, 0 <= self_state_dim <= input_dim, else EBC_ERR_UNSUPPORTED and ebc_last_error names the limit; lstm_input_dim
 * must be mlp1's last width (n_mlp1 = 0: input_dim), else EBC_ERR_INVALID.
 * The packed image (weights, and the gradient alike): mlp1's layers, then w_ih[k][4 H] (gate row q of input k at
 * k * 4 H + q), w_hh[k][4 H], b_ih[4 H], b_hh[4 H], then mlp's layers; a Linear layer as W[k][Op] — unit u of input k at
 * k * Op + u, Op = the layer's units padded to a multiple of 4 — followed by bias[Op]; pad entries are exactly 0.  b_ih and
 * b_hh are two tensors that receive the same gradient.  87 248 floats at the reference's widths with mlp1, 47 268 without. */
#define EBC_LSTM_NET_LAYERS 8
typedef struct EbcLstmNetWeights {
  uint32_t struct_size;
  int32_t n_mlp1, n_mlp;                      /* 0 or 4, 4 */
  int32_t self_state_dim;
  int32_t input_dim;                          /* the row width T */
  int32_t lstm_input_dim, hidden_dim;         /* I, H */
  int32_t reserved;
  int32_t widths[EBC_LSTM_NET_LAYERS];        /* the Linear layers' units */
  const float *weight[EBC_LSTM_NET_LAYERS];   /* host float32 [out][in] */
  const float *bias[EBC_LSTM_NET_LAYERS];     /* host float32 [out] */
  const float *w_ih, *w_hh, *b_ih, *b_hh;     /* host float32, nn.LSTM's layout */
} EbcLstmNetWeights;
/* One ebc_lstm_grad over B states of R row slots each:
 *   n            = n_valid[b] clamped to [0, R] (NULL: R); rows at or past n are never read and receive nothing
 *   value[b]     = the network's output on the state's rows [0, n); NaN without rows
 *   joint[b]     = mlp's input: the first self_state_dim floats of row 0, then h_n; zeros without rows
 *   live         = (sample_mask == NULL or sample_mask[b] != 0) and n >= 1; a state that is not live enters no sum (a
 *                  selection: its NaNs reach nothing but its own value and joint); a NaN inside a live state reaches
 *                  loss_sum and grad
 *   loss_sum     = the sum over the live states of (value - target)^2, count = their number
 *   grad         = d/dweights of grad_scale / 2 * loss_sum (grad_scale = 2 / count: torch's MSELoss), packed layout
 * The batch is cut into chunks of 4 consecutive states; inside a chunk a weight's sum is a float32 fmaf chain over the
 * live states and their steps ascending, the chunks are added ascending in float64 and rounded once: the result depends on
 * the inputs alone.  Every NaN written is the quiet NaN 0x7fc00000 (float64: 0x7ff8000000000000).  Scratch belongs to
 * the network and grows on demand, exactly as ebc_sarl_grad's: at most ONE ebc_lstm_grad in flight per network.  Device
 * pointers.  1 <= R <= ebc_lstm_net_grad_max_rows (a chunk's activations must fit a workgroup's 160 KB of LDS: 12 at the
 * reference widths with mlp1, 26 without), else EBC_ERR_UNSUPPORTED with nothing written; T other than the network's row
 * width is EBC_ERR_INVALID; a stream under capture is refused with EBC_ERR_UNSUPPORTED.
 * states_per_pass = S: 0 is the call above.  4, 2 or 1 runs a chunk's states S at a time, exactly as EbcSarlGradArgs says:
 * 1 <= R <= ebc_lstm_net_grad_max_rows_at(S) (12, 25 and 52 at the reference widths with mlp1), the bytes of
 * states_per_pass = 0 whatever S, EBC_ERR_UNSUPPORTED by R, S and the limit above it, EBC_ERR_INVALID for any other value. */
typedef struct EbcLstmGradArgs {
  uint32_t struct_size;
  int32_t B, R, T;
  float grad_scale;
  int32_t states_per_pass;      /* 0 = the whole chunk at once; 4, 2, 1 = that many states of a chunk at a time */
  const float *rows;            /* device float32 [B][R][T] */
  const int64_t *n_valid;       /* device int64 [B]; NULL = all R rows */
  const float *target;          /* device float32 [B] */
  const uint8_t *sample_mask;   /* device uint8 [B]; NULL = every state counts */
  float *grad;                  /* device float32 [ebc_lstm_net_packed_floats] */
  double *loss_sum;             /* device float64 [1] */
  int64_t *count;               /* device int64 [1] */
  float *value;                 /* device float32 [B], or NULL */
  float *joint;                 /* device float32 [B][self_state_dim + H], or NULL */
} EbcLstmGradArgs;
int ebc_lstm_net_create(const EbcLstmNetWeights *weights, int device_id, void **net_out);
int ebc_lstm_net_destroy(void *net);
int ebc_lstm_net_packed_floats(void *net, int64_t *floats_out);
int ebc_lstm_net_get_packed(void *net, void *stream, float *dst_dev);
int ebc_lstm_net_set_packed(void *net, void *stream, const float *src_dev);
/* the largest R ebc_lstm_grad takes for this network with the whole chunk at once (states_per_pass = 0) */
int ebc_lstm_net_grad_max_rows(void *net, int *rows_out);
/* the same for a value of EbcLstmGradArgs.states_per_pass: 0, 4, 2 or 1 (anything else is EBC_ERR_INVALID) */
int ebc_lstm_net_grad_max_rows_at(void *net, int states_per_pass, int *rows_out);
int ebc_lstm_grad(void *net, void *stream, const EbcLstmGradArgs *args);

#ifdef __cplusplus
}
#endif
#endif /* EBCSIM_H */
