"""ctypes wrapper of the CPU checker (oracle/libebc_oracle.so).

TEST INFRASTRUCTURE, NOT PRODUCT: only tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg import this module.  ORCA parity is unpinned (see
ebc_oracle.h); everything else is pinned by tests/golden/.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.join(os.path.dirname(_HERE), "eb-cadrl_amd")
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from ebcsim import _abi  # noqa: E402  (struct layouts of include/ebcsim.h)

_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libebc_oracle.so")
        if not os.path.exists(path):
            build()
        _LIB = _declare(C.CDLL(path))
    return _LIB


def _declare(L):
    """argument / result types of the checker's entry points on a loaded library"""
    d, i = C.c_double, C.c_int
    pd = C.POINTER(C.c_double)
    L.orc_point_to_segment_dist.restype = d
    L.orc_point_to_segment_dist.argtypes = [d] * 6
    L.orc_collision_agent_robot.restype = i
    L.orc_collision_agent_robot.argtypes = [d] * 9 + [i] + [d] * 3 + [pd]
    L.orc_grid_collision.restype = i
    L.orc_grid_collision.argtypes = [C.c_void_p, i, d, d, d, d, d, C.c_void_p]
    L.orc_reward.restype = None
    L.orc_reward.argtypes = [C.c_void_p, C.c_void_p, d, d, d, C.c_void_p, C.c_void_p,
                             pd, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), pd]
    L.orc_linear.restype = None
    L.orc_linear.argtypes = [d] * 5 + [pd, pd]
    L.orc_orca.restype = None
    L.orc_orca.argtypes = [C.c_void_p] + [d] * 8 + [i] + [C.c_void_p] * 5 + [pd, pd]
    L.orc_rvo2_agent0.restype = None
    L.orc_rvo2_agent0.argtypes = [C.c_float, C.c_float, i, C.c_float, C.c_void_p, C.c_void_p,
                                  C.c_float, C.c_float, C.c_void_p, i, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
    L.orc_rotate_row.restype = None
    L.orc_rotate_row.argtypes = [C.c_void_p, i, i, C.c_void_p]
    L.orc_propagate_robot.restype = None
    L.orc_propagate_robot.argtypes = [C.c_void_p, i, d, d, d, C.c_void_p]
    L.orc_observe.restype = i
    L.orc_observe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_step.restype = i
    L.orc_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_lookahead.restype = i
    L.orc_lookahead.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_robot_orca.restype = i
    L.orc_robot_orca.argtypes = [C.c_void_p, C.c_void_p, d, C.c_void_p]
    L.orc_robot_orca_sim.restype = i
    L.orc_robot_orca_sim.argtypes = [C.c_void_p, C.c_void_p, d, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_set_threads.restype = i
    L.orc_set_threads.argtypes = [i]
    return L


def set_threads(n):
    """Threads orc_step spreads its envs over (1 = the scalar port, the default); returns the
    value in effect.  Only bench.py's all-cores CPU baseline raises it."""
    return int(lib().orc_set_threads(int(n)))


class OrcState(C.Structure):
    _fields_ = [("E", C.c_int32), ("N", C.c_int32), ("S", C.c_int32), ("G", C.c_int32)] + [
        (k, C.c_void_p) for k in (
            "n_humans", "px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type",
            "n_static", "spx", "spy", "sradius", "grid_scene", "robot", "global_time",
            "arrival_time", "done", "human_action")
    ] + [("P", C.c_int32), ("stride", C.c_int32)] + [
        (k, C.c_void_p) for k in (
            "cursor", "p_n_humans", "p_px", "p_py", "p_vx", "p_vy", "p_gx", "p_gy", "p_radius",
            "p_v_pref", "p_type", "p_n_static", "p_spx", "p_spy", "p_sradius", "p_grid", "p_robot")
    ]


def _ptr(a):
    return None if a is None else a.ctypes.data


# ---- scalar entry points (used by the golden-vector tests) -------------------

def point_to_segment_dist(x1, y1, x2, y2, x3, y3):
    return lib().orc_point_to_segment_dist(x1, y1, x2, y2, x3, y3)


def collision_agent_robot(h, r, kinematics, action, dt, dmin):
    """h = (px,py,vx,vy,radius); r = (px,py,theta,radius) -> (dmin, collision)"""
    dm = C.c_double(dmin)
    c = lib().orc_collision_agent_robot(h[0], h[1], h[2], h[3], h[4], r[0], r[1], r[2], r[3],
                                        kinematics, action[0], action[1], dt, C.byref(dm))
    return dm.value, bool(c)


def grid_collision(grid, G, map_size_m, map_resolution, px, py, radius, border=None):
    g = None if grid is None else np.ascontiguousarray(grid, dtype=np.uint64)
    b = None if border is None else np.ascontiguousarray(border, dtype=np.float64)
    return bool(lib().orc_grid_collision(_ptr(g), G, map_size_m, map_resolution, px, py, radius,
                                         _ptr(b)))


def reward(params, robot, action, global_time, dmin, coll):
    robot = np.ascontiguousarray(robot, dtype=np.float64)
    dmin = np.ascontiguousarray(dmin, dtype=np.float64)
    coll = np.ascontiguousarray(coll, dtype=np.int32)
    rw, dg = C.c_double(), C.c_double()
    dn, inf = C.c_uint8(), C.c_uint8()
    lib().orc_reward(C.addressof(params), _ptr(robot), action[0], action[1], global_time,
                     _ptr(dmin), _ptr(coll), C.byref(rw), C.byref(dn), C.byref(inf), C.byref(dg))
    return rw.value, bool(dn.value), int(inf.value), dg.value


def linear(px, py, gx, gy, v_pref):
    vx, vy = C.c_double(), C.c_double()
    lib().orc_linear(px, py, gx, gy, v_pref, C.byref(vx), C.byref(vy))
    return vx.value, vy.value


def orca(params, self_state, others):
    """self_state = (px,py,vx,vy,radius,gx,gy,v_pref); others [m][5] px,py,vx,vy,radius"""
    o = np.ascontiguousarray(others, dtype=np.float64).reshape(-1, 5)
    cols = [np.ascontiguousarray(o[:, k]) for k in range(5)]
    vx, vy = C.c_double(), C.c_double()
    lib().orc_orca(C.addressof(params), *[float(x) for x in self_state], len(o),
                   *[_ptr(c) for c in cols], C.byref(vx), C.byref(vy))
    return vx.value, vy.value


def rvo2_agent0(time_step, neighbor_dist, max_neighbors, time_horizon, pos, vel, radius,
                max_speed0, pref0, library=None):
    """pos/vel [n][2], radius [n] float32 state of an rvo2 simulator; returns agent 0's new velocity.
    library: a Traced().lib to count the branches taken (default: the plain checker)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    vel = np.ascontiguousarray(vel, dtype=np.float32)
    radius = np.ascontiguousarray(radius, dtype=np.float32)
    pref0 = np.ascontiguousarray(pref0, dtype=np.float32)
    out = np.zeros(2, np.float32)
    (library or lib()).orc_rvo2_agent0(time_step, neighbor_dist, max_neighbors, time_horizon, pos[0].ctypes.data,
                                       vel[0].ctypes.data, float(radius[0]), max_speed0, pref0.ctypes.data,
                                       len(pos) - 1, pos[1:].ctypes.data, vel[1:].ctypes.data,
                                       radius[1:].ctypes.data, out.ctypes.data)
    return float(out[0]), float(out[1])


TRACE_NAMES = ("line_colliding", "line_circle", "line_left_leg", "line_right_leg", "line_nan",
               "nb_truncated", "nb_out_of_range", "nb_none",
               "lp1_dir0", "lp1_dir1", "lp1_fail_discriminant", "lp1_fail_parallel", "lp1_fail_interval",
               "lp1_parallel_skip",
               "lp2_fail_at_0", "lp2_fail_at_1", "lp2_fail_at_2", "lp2_fail_at_3_or_more",
               "lp3_entered", "lp3_bodies", "lp3_most_bodies", "lp3_parallel_same", "lp3_parallel_opposite",
               "lp3_inner_fail", "agents")  # the ORC_TR_* enum of ebc_oracle.c, in its order


class Traced:
    """The checker compiled with -DORC_TRACE (make -C oracle trace) into `directory` and loaded beside the plain one:
    OracleEnv(..., library=t.lib) and rvo2_agent0(..., library=t.lib) count the RVO2 branches they take into
    t.counts() (lp3_most_bodies is a maximum, the others are sums) until t.reset().  Test infrastructure only."""

    def __init__(self, directory):
        so = os.path.join(os.path.abspath(directory), "libebc_oracle_trace.so")
        subprocess.check_call(["make", "-s", "-C", _HERE, "trace", "TRACE_SO=" + so])
        self.lib = _declare(C.CDLL(so))
        self.lib.orc_trace_count.restype = C.c_int
        assert self.lib.orc_trace_count() == len(TRACE_NAMES)
        self._counts = (C.c_longlong * len(TRACE_NAMES)).in_dll(self.lib, "orc_trace_counts")
        self.lib.orc_set_threads(1)

    def reset(self):
        for k in range(len(TRACE_NAMES)):
            self._counts[k] = 0

    def counts(self):
        return {name: int(self._counts[k]) for k, name in enumerate(TRACE_NAMES)}


def rotate_rows(rows15, with_agent_type, rotate_unicycle):
    rows15 = np.ascontiguousarray(rows15, dtype=np.float64).reshape(-1, 15)
    T = 17 if with_agent_type else 13
    out = np.zeros((len(rows15), T), dtype=np.float32)
    L = lib()
    for k in range(len(rows15)):
        L.orc_rotate_row(rows15[k].ctypes.data, int(with_agent_type), int(rotate_unicycle),
                         out[k].ctypes.data)
    return out


def propagate_robot(robot, kinematics, action, dt):
    robot = np.ascontiguousarray(robot, dtype=np.float64)
    out = np.zeros(9)
    lib().orc_propagate_robot(_ptr(robot), kinematics, action[0], action[1], dt, _ptr(out))
    return out


# ---- batched environment --------------------------------------------------------

class OracleEnv:
    """Same call surface as ebcsim.BatchedEnv, computed by the scalar C restatement."""

    def __init__(self, params, n_envs, max_humans, max_static, library=None):
        self.params = params
        self._lib = library  # None: the plain checker; Traced().lib: the one with branch counters
        self.E, self.N, self.S = n_envs, max_humans, max_static
        self.G = int(round(params.map_size_m / params.map_resolution))
        self.T = _abi.rot_width(params)
        self.R = self.N + self.S
        E, N, S = self.E, self.N, max(self.S, 1)
        f = lambda *s: np.zeros(s, dtype=np.float64)  # noqa: E731
        self.a = dict(
            n_humans=np.zeros(E, np.int32), px=f(E, N), py=f(E, N), vx=f(E, N), vy=f(E, N),
            gx=f(E, N), gy=f(E, N), radius=f(E, N), v_pref=f(E, N),
            type=np.zeros((E, N), np.uint8), n_static=np.zeros(E, np.int32),
            spx=f(E, S), spy=f(E, S), sradius=f(E, S),
            grid_scene=np.arange(E, dtype=np.int32), robot=f(E, 9), global_time=f(E),
            arrival_time=f(E, N), done=np.zeros(E, np.uint8), human_action=f(E, N, 2))
        self._st = OrcState()
        self._alloc_pool(0)

    _POOL_KEYS = ("n_humans", "px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type",
                  "n_static", "spx", "spy", "sradius", "grid", "robot")

    def _alloc_pool(self, P):
        """E reset slots + P custom scenes; the reset slots survive a re-allocation."""
        E, N, S = self.E, self.N, max(self.S, 1)
        f = lambda *s: np.zeros(s, dtype=np.float64)  # noqa: E731
        n = E + P
        new = dict(
            n_humans=np.zeros(n, np.int32), px=f(n, N), py=f(n, N), vx=f(n, N), vy=f(n, N),
            gx=f(n, N), gy=f(n, N), radius=f(n, N), v_pref=f(n, N), type=np.zeros((n, N), np.uint8),
            n_static=np.zeros(n, np.int32), spx=f(n, S), spy=f(n, S), sradius=f(n, S),
            grid=np.zeros((n, self.G, 2), np.uint64), robot=f(n, 9))
        if getattr(self, "pool", None) is not None:
            # an env in the middle of an episode on a pool scene keeps only that slot's index for its map: the
            # map moves to the env's own slot (not a restart source once a pool is installed) before the slots go
            gs = self.a["grid_scene"]
            self.pool["grid"][:E] = self.pool["grid"][gs]
            gs[:] = np.arange(E, dtype=np.int32)
            for k in new:
                new[k][:E] = self.pool[k][:E]
        else:
            self.pool_has_grid = False
        self.pool = new
        self.P, self.stride = P, 0
        if P == 0:
            self.cursor = np.arange(E, dtype=np.int32)

    def _fill(self, dst, scene, ids, with_scene_rows=True):
        for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type"):
            dst[k][ids] = getattr(scene, k)
        dst["n_humans"][ids] = scene.n_humans
        if self.S:
            dst["n_static"][ids] = scene.n_static
            dst["spx"][ids], dst["spy"][ids], dst["sradius"][ids] = scene.spx, scene.spy, scene.sradius
        if "grid" in dst:
            dst["grid"][ids] = scene.grid if scene.grid is not None else 0
        dst["robot"][ids] = scene.robot

    def set_scene_pool(self, scene, stride=None):
        P, E = scene.n, self.E
        self._alloc_pool(P)
        self._fill(self.pool, scene, E + np.arange(P))
        if scene.grid is not None:
            self.pool_has_grid = True
        self.stride = (E if stride is None else stride) % P
        self.cursor = (E + np.arange(E) % P).astype(np.int32)

    def _L(self):
        return self._lib or lib()

    def _state(self):
        st = self._st
        st.E, st.N, st.S, st.G = self.E, self.N, self.S, self.G
        for k, v in self.a.items():
            setattr(st, k, v.ctypes.data)
        st.P, st.stride = self.P, self.stride
        st.cursor = self.cursor.ctypes.data
        for k in self._POOL_KEYS:
            setattr(st, "p_" + k, self.pool[k].ctypes.data)
        if not self.pool_has_grid:
            st.p_grid = None
        return st

    def reset(self, scene, env_ids=None):
        ids = np.arange(scene.n) if env_ids is None else np.asarray(env_ids)
        a = self.a
        self._fill(a, scene, ids)
        a["global_time"][ids] = 0
        a["arrival_time"][ids] = 0
        a["done"][ids] = 0
        a["grid_scene"][ids] = ids
        self._fill(self.pool, scene, ids)  # reset slot e: restart source and home of env e's grid
        if scene.grid is not None:
            self.pool_has_grid = True
        if self.P == 0:
            self.cursor[ids] = ids

    def set_human_actions(self, act):
        self.a["human_action"][...] = np.asarray(act, dtype=np.float64).reshape(self.E, self.N, 2)

    def step(self, robot_action=None, human_policy=_abi.HUMAN_ORCA,
             robot_policy=_abi.ROBOT_EXTERNAL, flags=0, border=None):
        E, N, R, T = self.E, self.N, self.R, self.T
        out = dict(reward=np.zeros(E), done=np.zeros(E, np.uint8), info=np.zeros(E, np.uint8),
                   dmin=np.zeros((E, 3)), dist_to_goal=np.zeros(E),
                   robot_action_out=np.zeros((E, 2)), human_action=np.zeros((E, N, 2)),
                   ob=np.zeros((E, R, 5)), obs_rotated=np.zeros((E, R, T), np.float32))
        args = _abi.EbcStepArgs()
        args.struct_size = C.sizeof(args)
        args.location = _abi.HOST
        args.human_policy, args.robot_policy = human_policy, robot_policy
        if robot_action is not None:
            ra = np.ascontiguousarray(robot_action, dtype=np.float64).reshape(E, 2)
            args.robot_action = ra.ctypes.data
        if border is not None:
            b = np.ascontiguousarray(border, dtype=np.float64).reshape(4)
            args.border = b.ctypes.data
            flags |= _abi.FLAG_BORDER
        args.flags = flags
        for k, v in out.items():
            setattr(args, k, v.ctypes.data)
        rc = self._L().orc_step(C.addressof(self.params), C.addressof(self._state()), C.addressof(args))
        if rc != 0:
            raise RuntimeError("orc_step failed: %d" % rc)
        return out

    def lookahead(self, actions, human_policy=_abi.HUMAN_ORCA, flags=0, border=None,
                  want_rows=True):
        actions = np.ascontiguousarray(actions, dtype=np.float64).reshape(-1, 2)
        A, E, R, T = len(actions), self.E, self.R, self.T
        out = dict(reward=np.zeros((E, A)), done=np.zeros((E, A), np.uint8),
                   info=np.zeros((E, A), np.uint8), dmin=np.zeros((E, A, 3)),
                   next_ob=np.zeros((E, R, 5)))
        if want_rows:
            out["rows_rotated"] = np.zeros((E, A, R, T), np.float32)
        args = _abi.EbcLookaheadArgs()
        args.struct_size = C.sizeof(args)
        args.location = _abi.HOST
        args.human_policy, args.n_actions = human_policy, A
        args.actions = actions.ctypes.data
        if border is not None:
            b = np.ascontiguousarray(border, dtype=np.float64).reshape(4)
            args.border = b.ctypes.data
            flags |= _abi.FLAG_BORDER
        args.flags = flags
        for k, v in out.items():
            setattr(args, k, v.ctypes.data)
        rc = self._L().orc_lookahead(C.addressof(self.params), C.addressof(self._state()),
                                 C.addressof(args))
        if rc != 0:
            raise RuntimeError("orc_lookahead failed: %d" % rc)
        return out

    def observe(self):
        ob = np.zeros((self.E, self.R, 5))
        obs = np.zeros((self.E, self.R, self.T), np.float32)
        self._L().orc_observe(C.addressof(self.params), C.addressof(self._state()), ob.ctypes.data,
                          obs.ctypes.data)
        return ob, obs

    def robot_orca_sim(self, enable=True):
        """The checker's ebc_robot_orca_sim: a fresh persistent simulator per env (no simulator yet), or none."""
        if enable:
            self._sim = dict(rows=np.full(self.E, -1, np.int32), radius=np.zeros((self.E, self.R), np.float32),
                             self=np.zeros((self.E, 2), np.float32))
        else:
            self._sim = None

    def robot_orca_sim_state(self, state=None):
        """get (state None) / set the simulators: dict(rows [E], radius [E, R], self [E, 2])"""
        if state is None:
            return {k: v.copy() for k, v in self._sim.items()}
        self.robot_orca_sim(True)
        for k in self._sim:
            self._sim[k][...] = state[k]

    def robot_orca(self, safety_space=0.0):
        """ORCA.predict for the robot of every env (orc_robot_orca / orc_robot_orca_sim) -> actions [E, 2]."""
        act = np.zeros((self.E, 2))
        sim = getattr(self, "_sim", None)
        if sim is not None:
            rc = self._L().orc_robot_orca_sim(C.addressof(self.params), C.addressof(self._state()), float(safety_space),
                                          sim["rows"].ctypes.data, sim["radius"].ctypes.data, sim["self"].ctypes.data,
                                          act.ctypes.data)
        else:
            rc = self._L().orc_robot_orca(C.addressof(self.params), C.addressof(self._state()),
                                      float(safety_space), act.ctypes.data)
        if rc:
            raise RuntimeError("orc_robot_orca failed: %d" % rc)
        return act

    def step_k(self, K, keys=("reward", "done", "info", "state_rotated"), robot_action=None,
               human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=0, robot_safety_space=0.0):
        """The checker's ebc_step_k: K times [observe -> robot action -> step], outputs stacked [K, ...]."""
        out = {k: [] for k in keys}
        for k in range(K):
            if "state_rotated" in out:
                out["state_rotated"].append(self.observe()[1])
            if "n_rows" in out:
                out["n_rows"].append(self.row_counts())
            if robot_policy == _abi.ROBOT_ORCA:
                act = self.robot_orca(robot_safety_space)
                o = self.step(robot_action=act, human_policy=human_policy, flags=flags)
                o["robot_action_out"] = act
            elif robot_policy == _abi.ROBOT_EXTERNAL:
                o = self.step(robot_action=np.asarray(robot_action)[k], human_policy=human_policy, flags=flags)
            else:
                o = self.step(human_policy=human_policy, robot_policy=_abi.ROBOT_LINEAR, flags=flags)
            for key in keys:
                if key not in ("state_rotated", "n_rows"):
                    out[key].append(o[key])
        return {k: np.stack(v) for k, v in out.items()}

    def row_counts(self):
        """Observation rows that exist per env (the checker's ebc_row_counts)."""
        return self.a["n_humans"].astype(np.int64) + (self.a["n_static"].astype(np.int64) if self.S else 0)

    def get_state(self):
        keys = ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type", "n_humans",
                "robot", "global_time", "arrival_time", "done")
        return {k: self.a[k].copy() for k in keys}
