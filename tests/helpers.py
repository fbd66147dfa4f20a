"""Shared helpers for the parity tests: fixture loading and scene/params rebuilds."""
import json
import os

import numpy as np

from ebcsim import _abi, config as ebc_config
from ebcsim.scene import SceneBatch, pack_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def params_of(z, key="params"):
    return ebc_config.params_from_dict(json.loads(str(z[key])))


def batch_from_init(z, prefix="init_", copies=1, max_humans=None, max_static=None):
    """SceneBatch from the init_* arrays a trajectory fixture stores (one scene, tiled)."""
    n = len(z[prefix + "px"])
    st = z[prefix + "static"].reshape(-1, 3)
    N = max_humans or n
    S = max_static if max_static is not None else len(st)
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = SceneBatch(copies, N, S, np.full(copies, n, np.int32), f(copies, N), f(copies, N),
                   f(copies, N), f(copies, N), f(copies, N), f(copies, N), f(copies, N),
                   f(copies, N), np.zeros((copies, N), np.uint8),
                   np.full(copies, len(st), np.int32), f(copies, max(S, 1)), f(copies, max(S, 1)),
                   f(copies, max(S, 1)), None, f(copies, 9))
    for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type"):
        getattr(b, k)[:, :n] = z[prefix + k]
    if len(st):
        b.spx[:, :len(st)], b.spy[:, :len(st)], b.sradius[:, :len(st)] = st.T
    grid = z[prefix + "grid"]
    if grid.any():
        b.grid = np.repeat(pack_grid(1.0 - grid)[None], copies, axis=0)
    b.robot[:] = z[prefix + "robot"]
    return b


HUMAN_POLICY = {"linear": _abi.HUMAN_LINEAR}


def human_policy_of(z):
    meta = json.loads(str(z["meta"]))
    return _abi.HUMAN_LINEAR if meta["human_policy"] == "linear" else _abi.HUMAN_ORCA


TRAJ_PINNED = ["traj_a5_linear", "traj_a5_scripted", "traj_a3b3s2_scripted", "traj_n10_walls_t17",
               "traj_unicycle_rotpen",
               "traj_a5_linear_dt01", "traj_unicycle_dt05"]  # time_step 0.1 (to the time-out at 3 s) and 0.5
TRAJ_ORCASUB = ["traj_a5_linear_orcasub", "traj_a5_scripted_orcasub",
                "traj_a3b3s2_scripted_orcasub", "traj_n10_walls_t17_orcasub",
                "traj_a3b3s2_dt01_orcasub"]  # time_step 0.1, the humans' horizon 2 and safety space 0.1
# the imitation-learning demonstrator: the robot itself on ORCA (rl/train.py:99-143)
TRAJ_IL = ["traj_a5_il_orcasub", "traj_n10_walls_il_orcasub"]


def check_trajectory(env, z, atol=1e-9, rot_atol=1e-5, lookahead=True):
    """Replay fixture `z` on `env` (OracleEnv or BatchedEnv; env 0 is compared; every env of
    the batch gets the same scene and actions) and assert parity step by step."""
    pol = human_policy_of(z)
    E = env.E
    n = len(z["init_px"])
    ns = len(z["init_static"].reshape(-1, 3))
    la_steps = list(z["la_step"]) if ("la_step" in z.files and lookahead) else []
    meta = json.loads(str(z["meta"]))
    robot_orca = meta.get("robot_mode") == "orca"
    for t in range(len(z["action"])):
        if robot_orca:
            # the demonstrator's action (Robot.act -> ORCA.predict) and the state the explorer keeps
            # for the imitation-learning memory (policy.last_state, transformed)
            a = env.robot_orca(meta["il_safety_space"])
            np.testing.assert_allclose(a[0], z["action"][t], atol=atol, rtol=0, err_msg="robot ORCA, step %d" % t)
            assert (a == a[0:1]).all()
            np.testing.assert_allclose(env.observe()[1][0][:n + ns], z["il_state"][t], atol=rot_atol,
                                       rtol=rot_atol, err_msg="IL state, step %d" % t)
        if t in la_steps:
            k = la_steps.index(t)
            la = env.lookahead(z["la_actions"], human_policy=pol)
            np.testing.assert_array_equal(la["done"][0].astype(bool), z["la_done"][k].astype(bool))
            np.testing.assert_array_equal(la["info"][0], z["la_info"][k])
            np.testing.assert_allclose(la["reward"][0], z["la_reward"][k], atol=atol, rtol=0)
            np.testing.assert_allclose(la["next_ob"][0][:n + ns], z["la_next_ob"][k][:, :5],
                                       atol=atol, rtol=0)
            np.testing.assert_allclose(la["rows_rotated"][0][:, :n + ns], z["la_rows"][k],
                                       atol=rot_atol, rtol=rot_atol)
        act = np.tile(z["action"][t], (E, 1))
        out = env.step(robot_action=act, human_policy=pol)
        msg = "step %d" % t
        assert bool(out["done"][0]) == bool(z["done"][t]), msg
        assert int(out["info"][0]) == int(z["info"][t]), msg
        np.testing.assert_allclose(out["reward"][0], z["reward"][t], atol=atol, rtol=0, err_msg=msg)
        np.testing.assert_allclose(out["dmin"][0], z["dmin"][t], atol=atol, rtol=0, err_msg=msg)
        if not np.isnan(z["dist_to_goal"][t]):
            np.testing.assert_allclose(out["dist_to_goal"][0], z["dist_to_goal"][t], atol=atol,
                                       rtol=0, err_msg=msg)
        np.testing.assert_allclose(out["human_action"][0][:n], z["human_action"][t], atol=atol,
                                   rtol=0, err_msg=msg)
        np.testing.assert_allclose(out["ob"][0][:n + ns], z["ob"][t][:, :5], atol=atol, rtol=0,
                                   err_msg=msg)
        np.testing.assert_allclose(out["obs_rotated"][0][:n + ns], z["rot"][t], atol=rot_atol,
                                   rtol=rot_atol, err_msg=msg)
        st = env.get_state()
        np.testing.assert_allclose(st["robot"][0], z["robot"][t], atol=atol, rtol=0, err_msg=msg)
        np.testing.assert_allclose(st["global_time"][0], z["time"][t], atol=1e-12, rtol=0)
        np.testing.assert_allclose(st["arrival_time"][0][:n], z["arrival"][t], atol=1e-12, rtol=0,
                                   err_msg=msg)
        hum = np.stack([st["px"][0][:n], st["py"][0][:n], st["vx"][0][:n], st["vy"][0][:n]], 1)
        np.testing.assert_allclose(hum, z["humans"][t], atol=atol, rtol=0, err_msg=msg)
        if E > 1:  # every replica of the scene must agree with env 0
            for key in ("reward", "info", "obs_rotated"):
                assert (out[key] == out[key][0:1]).all(), msg


def config_text_of(meta):
    """The INI text a trajectory fixture ran with: the scenes fixture's text of the same config file plus the
    overrides recorded in the fixture's meta."""
    import configparser
    import io
    zs = load("scenes")
    for k in range(int(zs["n"])):
        m = json.loads(str(zs["meta_%d" % k]))
        if m["config"] == meta["config"]:
            cfg = configparser.RawConfigParser()
            cfg.read_string(m["config_text"])
            for key, val in meta["overrides"].items():
                sec, opt = key.split(".")
                if sec in ("adults", "bicycles", "children") and opt == "policy":
                    continue
                cfg.set(sec, opt, str(val))
            buf = io.StringIO()
            cfg.write(buf)
            return buf.getvalue()
    raise KeyError(meta["config"])


def pool_reinstall_run(envs, E=24, steps=(60, 40, 60)):
    """ebc_set_scene_pool on a RUNNING batch (walls: every scene has its own occupancy grid): install 3 E scenes,
    step until envs have restarted from them, replace the pool by a SMALLER one (E / 2 scenes), keep stepping, then
    by a larger one.  Every env of `envs` gets the same calls; yields (phase, step, [outputs per env]) and checks,
    on envs[-1] after each re-installation, that every env still collides against the map of the scene whose
    static rows it holds — the env must not follow the pool's slots."""
    import configparser
    from ebcsim import scene as ebc_scene
    z = load("traj_n10_walls_t17_orcasub")
    meta = json.loads(str(z["meta"]))
    params = params_of(z)
    params.time_limit = 4  # short episodes: many restarts
    cfg = configparser.RawConfigParser()
    cfg.read_string(config_text_of(meta))
    sc = ebc_scene.SceneConfig.from_config(cfg)
    gen = lambda seeds: [ebc_scene.generate_scene(sc, int(s)) for s in seeds]  # noqa: E731
    all_scenes = {}

    def batch(seeds, N=None, S=None):
        b = ebc_scene.SceneBatch.from_scenes(gen(seeds), N, S)
        for c in range(b.n):
            all_scenes[b.spx[c].tobytes() + b.spy[c].tobytes()] = b.grid[c].copy()
        return b
    first = batch(range(7000, 7000 + E), None, 12)
    N, S = first.N, first.S
    pools = [batch(range(7100, 7100 + 3 * E), N, S), batch(range(7300, 7300 + E // 2), N, S),
             batch(range(7400, 7400 + 5 * E), N, S)]
    made = [mk(params, E, N, S) for mk in envs]
    for env in made:
        env.reset(first)
    probe = made[-1]
    restarts = 0
    for phase, pool in enumerate(pools):
        for env in made:
            env.set_scene_pool(pool, stride=E)
        if hasattr(probe, "pool"):  # the oracle: white box
            gs = probe.a["grid_scene"]
            for e in range(E):
                key = probe.a["spx"][e].tobytes() + probe.a["spy"][e].tobytes()
                np.testing.assert_array_equal(probe.pool["grid"][gs[e]], all_scenes[key], err_msg="phase %d env %d" % (phase, e))
        for t in range(steps[phase]):
            outs = [env.step(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET)
                    for env in made]
            restarts += int(outs[-1]["done"].sum())
            yield phase, t, outs
    assert restarts > 4 * E
    yield -1, 0, [env.get_state() for env in made]


class CpuDeviceEnv(object):
    """The *_device call surface of ebcsim.batched.BatchedEnv on CPU torch tensors, computed by the
    oracle: lets the trainer's schedule (ebcsim/train.py: collect, collect_il, run_training — host
    logic over that surface) run under gloo without a GPU.  Test scaffolding only."""

    def __init__(self, params, E, N, S):
        from oracle import oracle
        self._o = oracle.OracleEnv(params, E, N, S)
        self.params, self.E, self.N, self.S, self.R, self.T = params, E, N, S, N + S, self._o.T
        self.device = 0
        self.ragged = False
        self.steps = 0

    def _note(self, scene):
        rows = np.asarray(scene.n_humans, np.int64) + (np.asarray(scene.n_static, np.int64) if self.S else 0)
        self.ragged = bool(self.ragged or (rows < self.R).any())

    def reset(self, scene, env_ids=None):
        self._o.reset(scene, env_ids)
        self._note(scene)

    def set_scene_pool(self, scene, stride=None):
        self._o.set_scene_pool(scene, stride)
        self._note(scene)

    def get_state(self):
        return self._o.get_state()

    def use_torch_stream(self):
        pass

    def synchronize(self):
        pass

    def alloc_step_outputs(self, keys=("reward", "done", "info", "obs_rotated")):
        import torch
        E, N, R, T = self.E, self.N, self.R, self.T
        shapes = dict(reward=((E,), torch.float64), done=((E,), torch.uint8), info=((E,), torch.uint8),
                      dmin=((E, 3), torch.float64), dist_to_goal=((E,), torch.float64),
                      obs_rotated=((E, R, T), torch.float32))
        return {k: torch.zeros(shapes[k][0], dtype=shapes[k][1]) for k in keys}

    def alloc_lookahead_outputs(self, n_actions, keys=("reward", "done", "info", "rows_rotated")):
        import torch
        E, R, T, A = self.E, self.R, self.T, int(n_actions)
        shapes = dict(reward=((E, A), torch.float64), done=((E, A), torch.uint8), info=((E, A), torch.uint8),
                      rows_rotated=((E, A, R, T), torch.float32))
        return {k: torch.zeros(shapes[k][0], dtype=shapes[k][1]) for k in keys}

    def step_device(self, outputs, robot_action=None, human_policy=_abi.HUMAN_ORCA,
                    robot_policy=_abi.ROBOT_EXTERNAL, flags=0):
        import torch
        out = self._o.step(robot_action=None if robot_action is None else robot_action.numpy(),
                           human_policy=human_policy, robot_policy=robot_policy, flags=flags)
        for k, t in outputs.items():
            t.copy_(torch.from_numpy(out[k]))
        self.steps += 1

    def lookahead_device(self, actions, outputs, human_policy=_abi.HUMAN_ORCA, flags=0):
        import torch
        out = self._o.lookahead(actions.numpy(), human_policy=human_policy, flags=flags)
        for k, t in outputs.items():
            t.copy_(torch.from_numpy(out[k]))

    def observe_device(self, obs_rotated):
        import torch
        obs_rotated.copy_(torch.from_numpy(self._o.observe()[1]))

    def row_counts_device(self, n_rows):
        import torch
        n_rows.copy_(torch.from_numpy(self._o.row_counts()))

    def alloc_step_k_outputs(self, K, keys=("reward", "done", "info", "state_rotated")):
        import torch
        E, R, T = self.E, self.R, self.T
        shapes = dict(state_rotated=((E, R, T), torch.float32), n_rows=((E,), torch.int64),
                      robot_action_out=((E, 2), torch.float64), reward=((E,), torch.float64), done=((E,), torch.uint8),
                      info=((E,), torch.uint8), dmin=((E, 3), torch.float64), dist_to_goal=((E,), torch.float64),
                      obs_rotated=((E, R, T), torch.float32))
        return {k: torch.zeros((K,) + shapes[k][0], dtype=shapes[k][1]) for k in keys}

    def step_k_device(self, outputs, K, robot_action=None, human_policy=_abi.HUMAN_ORCA,
                      robot_policy=_abi.ROBOT_LINEAR, flags=0, robot_safety_space=0.0):
        import torch
        out = self._o.step_k(K, tuple(outputs), None if robot_action is None else robot_action.numpy(), human_policy,
                             robot_policy, flags, robot_safety_space)
        for k, t in outputs.items():
            t.copy_(torch.from_numpy(out[k]))
        self.steps += K

    def robot_orca_sim(self, enable=True):
        self._o.robot_orca_sim(enable)

    def robot_orca_device(self, actions, safety_space=0.0):
        import torch
        actions.copy_(torch.from_numpy(self._o.robot_orca(safety_space)))


def il_persistent_episodes(name, copies=1):
    """(z, params, N, S, [SceneBatch per episode]) of an il_persistent_* fixture."""
    z = load(name)
    K = int(z["n_episodes"])
    N = max(len(z["init%d_px" % k]) for k in range(K))
    S = max(len(z["init%d_static" % k].reshape(-1, 3)) for k in range(K))
    return z, params_of(z), N, S, [batch_from_init(z, prefix="init%d_" % k, copies=copies, max_humans=N, max_static=S)
                                    for k in range(K)]


def check_il_persistent(make_env, name, copies=1):
    """Consecutive imitation-learning episodes on ONE ORCA policy object (the reference's Explorer.run_k_episodes on
    its il_policy, rl/train.py:130-133): with the persistent simulator enabled once and env.reset() per episode the
    robot's actions, rewards and terminal classes are the reference's in EVERY episode; without it they are not."""
    z, params, N, S, batches = il_persistent_episodes(name, copies)
    safety = float(z["safety_space"])
    tile = lambda b: b  # noqa: E731
    env = make_env(params, copies, N, S)
    env.robot_orca_sim(True)
    for k, b in enumerate(batches):
        env.reset(tile(b))
        for t in range(len(z["action%d" % k])):
            a = env.robot_orca(safety)
            np.testing.assert_allclose(a[0], z["action%d" % k][t], atol=1e-9, rtol=0, err_msg="episode %d step %d" % (k, t))
            assert (a == a[0:1]).all()
            out = env.step(robot_action=a, human_policy=_abi.HUMAN_ORCA)
            np.testing.assert_allclose(out["reward"][0], z["reward%d" % k][t], atol=1e-9, rtol=0)
            assert int(out["info"][0]) == int(z["info%d" % k][t]), (k, t)
        assert bool(out["done"][0])
    # the fixture has teeth: a fresh simulator per call departs from the reference once the radii have changed
    if not bool(z["sim_rebuilt"][1:].all()):
        env.robot_orca_sim(False)
        differs = False
        for k, b in enumerate(batches[:2]):
            env.reset(tile(b))
            for t in range(len(z["action%d" % k])):
                a = env.robot_orca(safety)
                differs = differs or not np.allclose(a[0], z["action%d" % k][t], atol=1e-9, rtol=0)
                env.step(robot_action=np.tile(z["action%d" % k][t], (copies, 1)), human_policy=_abi.HUMAN_ORCA)
        assert differs


def reference_rule(row):
    """The reference's choice of an action from its values, as it runs it (rl/policy/multi_human_rl.py:36-80): a scalar
    loop from max_value = -inf that takes an action when `value > max_value` — so the first maximum wins, a NaN is never
    taken, and a row with no value above -inf leaves max_action None, which raises."""
    max_value = float("-inf")
    max_action = None
    for action, value in enumerate(row):
        if value > max_value:
            max_value = value
            max_action = action
    if max_action is None:
        raise ValueError("Value network is not well trained. ")
    return max_action


class Guarded:
    """A device buffer of any shape and dtype with a canary on each side, for the outputs a kernel writes.  Each canary is
    at least 64 KiB and at least 8 row tiles of the buffer (8 * tile_rows rows: the span of one workgroup), so a write
    past either end lands in a canary instead of the caching allocator's slack.  With poison (the default) the inside
    starts as a byte pattern no kernel writes, and check() asserts that every element was overwritten — for buffers whose
    contract says every element is written.  `t` is the view the kernel gets."""
    CANARY, POISON = 0xB6, 0xA5

    def __init__(self, shape, dtype, tile_rows=32, poison=True, device="cuda"):
        import torch
        self.shape = tuple(int(s) for s in shape)
        self.isz = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.isz
        row = int(np.prod(self.shape[1:], dtype=np.int64)) * self.isz
        self.pad = -(-max(64 << 10, 8 * tile_rows * row) // 256) * 256  # the inside keeps the allocation's alignment
        self.raw = torch.full((2 * self.pad + self.nbytes,), self.CANARY, dtype=torch.uint8, device=device)
        self.poison = bool(poison)
        if poison:
            self.raw[self.pad:self.pad + self.nbytes].fill_(self.POISON)
        self.t = self.raw[self.pad:self.pad + self.nbytes].view(dtype).view(self.shape)
        self.ptr = self.raw.data_ptr() + self.pad  # the inside's address, also when it is empty (t.data_ptr() is 0 then)
        self.np_dtype = torch.empty((), dtype=dtype).numpy().dtype

    def check(self, written=None):
        """Asserts both canaries are intact; written (default: whether the buffer was poisoned) asserts that no element
        still holds the poison, written=False that every one does (nothing written).  -> the inside on the host."""
        b = self.raw.cpu().numpy()
        lo, inside, hi = b[:self.pad], b[self.pad:self.pad + self.nbytes], b[self.pad + self.nbytes:]
        bad = np.nonzero(lo != self.CANARY)[0]
        assert not len(bad), "write before the buffer %s: %d canary bytes, the first %d bytes before it" % (
            self.shape, len(bad), self.pad - bad[0])
        bad = np.nonzero(hi != self.CANARY)[0]
        assert not len(bad), "write past the end of the buffer %s: %d canary bytes, the last %d bytes after it" % (
            self.shape, len(bad), bad[-1] + 1)
        if written is None:
            written = self.poison if self.poison else None
        if written is not None:
            assert self.poison, "check(written=...) needs a poisoned buffer"
            untouched = (inside.reshape(-1, self.isz) == self.POISON).all(1)
            if written:
                assert not untouched.any(), "%d of %d elements of %s not written (the first: %d)" % (
                    int(untouched.sum()), len(untouched), self.shape, int(np.argmax(untouched)))
            else:
                assert untouched.all(), "%d elements of %s written" % (int((~untouched).sum()), self.shape)
        return inside.view(self.np_dtype).reshape(self.shape)


# ---- batches that drive the ORCA solver into every branch (tests/test_orca_branches_cpu.py asserts from the traced
# oracle that they do; tests/test_orca_branches_gpu.py holds the kernels to the oracle on the same batches) ----------

ORCA_GROUP_SIZES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32)  # kGroupSizes of csrc/ebcsim.hip


def orca_group_size(others):
    return next((g for g in ORCA_GROUP_SIZES if g >= others), 32)


def _blank_batch(E, N, S):
    f = lambda *s: np.zeros(s)  # noqa: E731
    b = SceneBatch(E, N, S, np.full(E, N, np.int32), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                   f(E, N), np.zeros((E, N), np.uint8), np.full(E, S, np.int32), f(E, max(S, 1)), f(E, max(S, 1)),
                   f(E, max(S, 1)), None, f(E, 9))
    b.robot[:] = [0.0, -30.0, 0.0, 0.0, 0.3, 0.0, 30.0, 0.7, np.pi / 2]  # out of everyone's range
    return b


def _ragged(rs, b):
    """A third of the envs hold 0..N humans (0..S static rows): empty lanes inside groups, empty envs."""
    for e in range(2, b.n, 3):
        b.n_humans[e] = rs.randint(0, b.N + 1)
        if b.S:
            b.n_static[e] = rs.randint(0, b.S + 1)


def _clear_unused(b):
    for e in range(b.n):
        for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref"):
            getattr(b, k)[e, b.n_humans[e]:] = 0
        for k in ("spx", "spy", "sradius"):
            getattr(b, k)[e, b.n_static[e]:] = 0


def orca_crowd(rs, E, N, box, S=0, robot_inside=False):
    """Positions and goals uniform in [-box, box]^2, velocities in +-0.5, radius U(0.1, 0.5), v_pref U(0.3, 1.2); static
    rows drawn like the positions, three in ten on top of a human; the robot, when it takes part, drawn like a human."""
    b = _blank_batch(E, N, S)
    _ragged(rs, b)
    for k in ("px", "py", "gx", "gy"):
        getattr(b, k)[:] = rs.uniform(-box, box, (E, N))
    b.vx[:], b.vy[:] = rs.uniform(-0.5, 0.5, (E, N)), rs.uniform(-0.5, 0.5, (E, N))
    b.radius[:], b.v_pref[:] = rs.uniform(0.1, 0.5, (E, N)), rs.uniform(0.3, 1.2, (E, N))
    if S:
        b.spx[:], b.spy[:] = rs.uniform(-box, box, (E, S)), rs.uniform(-box, box, (E, S))
        b.sradius[:] = rs.uniform(0.1, 0.5, (E, S))
        for e in range(E):
            for j in range(S):
                if b.n_humans[e] and rs.uniform() < 0.3:
                    i = rs.randint(b.n_humans[e])
                    b.spx[e, j], b.spy[e, j] = b.px[e, i], b.py[e, i]
    if robot_inside:
        b.robot[:, 0:2] = rs.uniform(-box, box, (E, 2))
        b.robot[:, 2:4] = rs.uniform(-0.5, 0.5, (E, 2))
        b.robot[:, 5:7] = rs.uniform(-box, box, (E, 2))
    _clear_unused(b)
    return b


def orca_lattice(rs, E, N, spacing, S=0, robot_inside=False):
    """Humans (then the robot, then the static rows while free cells last) on distinct cells of the smallest square
    lattice that holds them, centred on the origin; spacing 0.5 or 0.75 is exact in float32, so squared distances tie
    exactly and ORCA lines come out parallel.  Radius 0.3, v_pref 1, goal = -position, velocity = the unit vector to the
    goal.  Both sides under test rank equal distances in insertion order; RVO2's kd-tree order for >= 11 agents is not
    modelled."""
    b = _blank_batch(E, N, S)
    _ragged(rs, b)
    side = int(np.ceil(np.sqrt(N + int(robot_inside))))
    cells = (np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2) - (side - 1) / 2.0) * spacing

    def heading(p):
        n = np.hypot(p[..., 0], p[..., 1])[..., None]
        return np.where(n > 0, -p / np.where(n > 0, n, 1), 0.0)
    for e in range(E):
        order = rs.permutation(len(cells))
        pos = cells[order[:N]]
        b.px[e], b.py[e] = pos.T
        b.gx[e], b.gy[e] = -pos.T
        b.vx[e], b.vy[e] = heading(pos).T
        rest = list(order[N:])
        if robot_inside:
            c = cells[rest.pop(0)]
            b.robot[e, 0:2], b.robot[e, 5:7], b.robot[e, 2:4] = c, -c, heading(c) * 0.7
        for j in range(S):  # on a free cell, else on top of a human
            c = cells[rest.pop(0)] if rest else pos[rs.randint(N)]
            b.spx[e, j], b.spy[e, j] = c
    b.radius[:], b.v_pref[:] = 0.3, 1.0
    b.sradius[:] = 0.3 if S else 0.0
    _clear_unused(b)
    return b


def orca_twins(rs, E, N, box, prob=0.3, S=0, robot_inside=False):
    """orca_crowd in which each human i >= 1 (and the robot, when it takes part) copies, with probability prob, the
    position and radius of a random earlier human; half of those copy its velocity too: relative position AND velocity
    zero, w = 0, a NaN ORCA line.  The others keep their own: a finite line from a zero relative position."""
    b = orca_crowd(rs, E, N, box, S, robot_inside)
    for e in range(E):
        n = int(b.n_humans[e])
        for i in list(range(1, n)) + ([N] if robot_inside and n else []):
            if rs.uniform() < prob:
                k = rs.randint(min(i, n))
                same_velocity = rs.uniform() < 0.5
                if i < N:
                    b.px[e, i], b.py[e, i], b.radius[e, i] = b.px[e, k], b.py[e, k], b.radius[e, k]
                    if same_velocity:
                        b.vx[e, i], b.vy[e, i] = b.vx[e, k], b.vy[e, k]
                else:
                    b.robot[e, 0:2] = b.px[e, k], b.py[e, k]
                    if same_velocity:
                        b.robot[e, 2:4] = b.vx[e, k], b.vy[e, k]
    return b


def concat_batches(parts):
    b = _blank_batch(sum(p.n for p in parts), parts[0].N, parts[0].S)
    for k in ("n_humans", "px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type", "n_static", "spx", "spy",
              "sradius", "robot"):
        setattr(b, k, np.concatenate([getattr(p, k) for p in parts]))
    return b


def orca_branch_batch(seed, N, lanes, S=0, robot_inside=False):
    """One batch for one (N, S): crowd(4), crowd(1), lattice(0.5), lattice(0.75) and twins(1.5) one after the other, 24 to
    32 envs each.  `lanes` is the ORCA group size the batch is meant for: the number of envs is odd and, where such a
    number exists, neither it nor the number of humans is a multiple of the groups per wave (64 // lanes), so the
    last wave of a launch is partly filled."""
    rs = np.random.RandomState(seed)
    per_wave = 64 // lanes
    sizes = [(c, c2) for c in range(27, 33) for c2 in range(24, 33) if (4 * c + c2) % 2 == 1]
    c, c2 = max(sizes, key=lambda s: int((4 * s[0] + s[1]) * N % per_wave != 0) + int((4 * s[0] + s[1]) % per_wave != 0))
    kw = dict(S=S, robot_inside=robot_inside)
    return concat_batches([orca_crowd(rs, c, N, 4.0, **kw), orca_crowd(rs, c, N, 1.0, **kw),
                           orca_lattice(rs, c, N, 0.5, **kw), orca_lattice(rs, c, N, 0.75, **kw),
                           orca_twins(rs, c2, N, 1.5, **kw)])


# (humans, robot_visible): every group size, each both full and with spare lanes
ORCA_HUMAN_COUNTS = [(n, 0) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 17, 18, 22, 23, 33)] + [(10, 1), (32, 1)]
# name -> (maxNeighbors, neighborDist, time_step, orca_time_horizon, orca_safety_space); the last three default to
# 0.25, 5 and 0, the values of every golden
ORCA_PARAM_SETS = {"default": (10, 10.0), "mn3-nd2": (3, 2.0), "mn1": (1, 10.0), "mn0": (0, 10.0),
                   "dt0.1": (10, 10.0, 0.1), "dt0.5": (10, 10.0, 0.5), "hor2": (10, 10.0, 0.25, 2.0),
                   "hor0.5": (10, 10.0, 0.25, 0.5), "saf0.1": (10, 10.0, 0.25, 5.0, 0.1),
                   "all": (3, 2.0, 0.1, 2.0, 0.1)}
ORCA_PARAM_SETS = {k: v + (0.25, 5.0, 0.0)[len(v) - 2:] for k, v in ORCA_PARAM_SETS.items()}
# the sets that move time_step, the ORCA horizon or the humans' safety space off the default, and where they run: the
# smallest group, a 5-lane group, the visible robot twice (the safety space goes onto ITS radius there), a group above ten
# others, the 32-lane group with 33 agents
ORCA_MOVED_SETS = ("dt0.1", "dt0.5", "hor2", "hor0.5", "saf0.1", "all")
ORCA_MOVED_COUNTS = [(2, 0), (6, 0), (10, 1), (14, 0), (32, 1)]
ORCA_HUMAN_CASES = ([(n, rv, ps) for n, rv in ORCA_HUMAN_COUNTS for ps in ("default", "mn3-nd2")]
                    + [(n, 0, ps) for n in (6, 13) for ps in ("mn1", "mn0")]
                    + [(n, rv, ps) for n, rv in ORCA_MOVED_COUNTS for ps in ORCA_MOVED_SETS])
# (humans, static rows) of the robot's own ORCA: rows 1..13, 16, 17, 21, 22, 32
ORCA_ROBOT_CASES = [(r, 0) for r in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 22)] + [(6, 4), (10, 11), (20, 12)]
# the robot's own solve under a handle whose safety space (the humans', 0.1) is not the robot's (0 / 0.15)
ORCA_ROBOT_MOVED_CASES = [(n, s, ps) for n, s in ((5, 0), (6, 4), (20, 12)) for ps in ("saf0.1", "all")]
ORCA_STEPS = 3


def orca_case_id(case):
    return "N%d%s-%s" % (case[0], "+robot" if case[1] else "", case[2]) if len(case) == 3 else "N%d-S%d" % case


def orca_robot_case_id(case):
    return "N%d-S%d" % case[:2] + "".join("-" + ps for ps in case[2:])


def orca_case_params(rv=0, param_set="default"):
    params = params_of(load("traj_n10_walls_t17_orcasub"))
    params.robot_visible = rv
    (params.orca_max_neighbors, params.orca_neighbor_dist, params.time_step, params.orca_time_horizon,
     params.orca_safety_space) = ORCA_PARAM_SETS[param_set]
    return params


_orca_batches = {}


def orca_human_batch(N, rv):
    """The batch of a human count: the same under every parameter set, for the CPU and the GPU tests alike."""
    if (N, rv) not in _orca_batches:
        _orca_batches[N, rv] = orca_branch_batch(52000 + 10 * N + rv, N, orca_group_size(max(N - 1 + rv, 1)),
                                                 robot_inside=bool(rv))
    return _orca_batches[N, rv]


def orca_robot_batch(N, S):
    if (N, S, "robot") not in _orca_batches:
        _orca_batches[N, S, "robot"] = orca_branch_batch(67000 + 100 * N + S, N, orca_group_size(N + S), S=S,
                                                         robot_inside=True)
    return _orca_batches[N, S, "robot"]


def orca_robot_actions(E):
    """The robot's supplied action of every step: [ORCA_STEPS, E, 2] from the holonomic action space."""
    from ebcsim import actions as ebc_actions
    space = ebc_actions.build_action_space(0.7)
    return space[np.random.RandomState(4242).randint(len(space), size=(ORCA_STEPS, E))]


_orca_refs = {}


def orca_reference(case, library=None):
    """What the oracle computes for a case of ORCA_HUMAN_CASES, once per session for the plain library: the outputs of
    ORCA_STEPS steps from reset under HUMAN_ORCA with the supplied robot actions, and the state after each."""
    from oracle import oracle
    if library is None and case in _orca_refs:
        return _orca_refs[case]
    N, rv, ps = case
    b = orca_human_batch(N, rv)
    o = oracle.OracleEnv(orca_case_params(rv, ps), b.n, N, 0, library=library)
    o.reset(b)
    act = orca_robot_actions(b.n)
    ref = dict(out=[], state=[])
    for t in range(ORCA_STEPS):
        ref["out"].append(o.step(robot_action=act[t], human_policy=_abi.HUMAN_ORCA))
        ref["state"].append(o.get_state())
    if library is None:
        for v in ref["out"] + ref["state"]:
            for a in v.values():
                a.flags.writeable = False
        _orca_refs[case] = ref
    return ref


def orca_robot_reference(case, safety, library=None):
    """robot_orca(safety) of a case (N, S), or (N, S, parameter set) of ORCA_ROBOT_MOVED_CASES, from reset."""
    from oracle import oracle
    N, S = case[:2]
    b = orca_robot_batch(N, S)
    o = oracle.OracleEnv(orca_case_params(0, *case[2:]), b.n, N, S, library=library)
    o.reset(b)
    return o.robot_orca(safety)


# ---- the robot side of a step: collision per type, dmin, reward, done, info (tests/test_robot_outcome_cpu.py asserts
# the recipes and the coverage on the oracle; tests/test_robot_outcome_gpu.py holds the four kernels that restate the
# reduction to the same answers) -----------------------------------------------------------------------------------

OUTCOME_FORMS = ("step", "orca", "lookahead", "one_launch")  # step_kernel, orca_step_kernel, lookahead_kernel, rollout_kernel
OUTCOME_KEYS = ("reward", "done", "info", "dmin", "dist_to_goal")
COLLISION_CODE = (_abi.INFO_COLLISION_ADULT, _abi.INFO_COLLISION_BICYCLE, _abi.INFO_COLLISION_CHILD)
LA_CHUNK = 127  # envs = actions of one look-ahead call: under the 128 the call takes, and no multiple of a wave
FAR_GOAL = 50.0


def outcome_params(kinematics=_abi.HOLONOMIC, dt=0.25, **kw):
    """Holonomic / unicycle parameters on the 9.0 m / 0.1 m map with an invisible robot; kw sets fields (tuples: arrays)."""
    import ctypes
    p = params_of(load("traj_n10_walls_t17_orcasub"))
    p.robot_kinematics, p.time_step, p.robot_visible, p.time_limit = kinematics, dt, 0, 25.0
    p.map_size_m, p.map_resolution = 9.0, 0.1
    for k, v in kw.items():
        setattr(p, k, (ctypes.c_double * len(v))(*v) if isinstance(v, (tuple, list)) else v)
    return p


def batch_rows(b, ids):
    """The envs `ids` of a batch as a batch of their own."""
    ids = np.asarray(ids)
    f = lambda a: np.ascontiguousarray(a[ids])  # noqa: E731
    return SceneBatch(len(ids), b.N, b.S, f(b.n_humans), f(b.px), f(b.py), f(b.vx), f(b.vy), f(b.gx), f(b.gy),
                      f(b.radius), f(b.v_pref), f(b.type), f(b.n_static), f(b.spx), f(b.spy), f(b.sradius),
                      None if b.grid is None else f(b.grid), f(b.robot))


def split_off_wave_multiples(ids):
    """`ids` as it is, or in two odd-sized parts when its length is a multiple of 4 (of the four-lanes-per-env packing,
    hence of every envs-per-wave count and of 64): every launch then ends in a part-filled wave."""
    ids = np.asarray(ids)
    if len(ids) % 4 or len(ids) < 4:
        return [ids]
    cut = len(ids) // 2 + (1 if (len(ids) // 2) % 2 == 0 else 0)
    return [ids[:cut], ids[cut:]]


def _close(env):
    if hasattr(env, "close"):
        env.close()


def robot_outcome_forms(make_env, params, b, act, border=None, forms=OUTCOME_FORMS):
    """One step of batch `b` under the supplied robot actions `act` [E, 2], from reset, once per form ->
    {form: {reward, done, info, dmin, dist_to_goal}} (the look-ahead has no dist_to_goal; the one-launch form takes no
    border and is left out when there is one).  The look-ahead runs LA_CHUNK envs at a time with the chunk's own
    actions as the action set, and the diagonal (env i, action i) is what it reports for env i."""
    E = b.n
    act = np.ascontiguousarray(act, dtype=np.float64).reshape(E, 2)
    res = {}
    env = make_env(params, E, b.N, b.S)
    for form in forms:
        if form == "lookahead" or (form == "one_launch" and border is not None):
            continue
        env.reset(b)
        if form == "step":
            o = env.step(robot_action=act, human_policy=_abi.HUMAN_LINEAR, border=border)
        elif form == "orca":
            o = env.step(robot_action=act, human_policy=_abi.HUMAN_ORCA, border=border)
        else:
            o = env.step_k(1, OUTCOME_KEYS, robot_action=act[None], human_policy=_abi.HUMAN_ORCA,
                           robot_policy=_abi.ROBOT_EXTERNAL, flags=_abi.FLAG_ONE_LAUNCH)
            o = {k: v[0] for k, v in o.items()}
        res[form] = {k: np.array(o[k]) for k in OUTCOME_KEYS}
    _close(env)
    if "lookahead" in forms:
        c = min(LA_CHUNK, E)
        env = make_env(params, c, b.N, b.S)
        parts = {k: [] for k in ("reward", "done", "info", "dmin")}
        for lo in range(0, E, c):
            ids = np.arange(lo, min(lo + c, E))
            m = len(ids)
            env.reset(batch_rows(b, ids))  # a short last chunk leaves the other envs on the chunk before
            a = np.concatenate([act[ids], np.repeat(act[ids][-1:], c - m, 0)])
            la = env.lookahead(a, human_policy=_abi.HUMAN_LINEAR, border=border, want_rows=False)
            d = np.arange(m)
            for k in parts:
                parts[k].append(la[k][d, d])
        _close(env)
        res["lookahead"] = {k: np.concatenate(v) for k, v in parts.items()}
    return res


def assert_forms_agree(res, tag):
    """reward, done, info, dmin (dist_to_goal where both have it): byte for byte between every two forms."""
    names = list(res)
    for name in names[1:]:
        for k in OUTCOME_KEYS:
            if k in res[names[0]] and k in res[name]:
                x, y = res[names[0]][k], res[name][k]
                assert x.shape == y.shape and x.astype(y.dtype).tobytes() == y.tobytes(), \
                    "%s: %s of %s and %s differ (first env %s)" % (tag, k, names[0], name, np.argwhere(
                        ~((x == y) | ((x != x) & (y != y))))[:1].tolist())


def assert_outcome(got, ref, tag, atol=1e-9):
    """done and info exact; reward, dmin and dist_to_goal at the project's 1e-9 (inf equal to inf)."""
    np.testing.assert_array_equal(got["done"].astype(bool), ref["done"].astype(bool), err_msg=tag + " done")
    np.testing.assert_array_equal(got["info"], ref["info"], err_msg=tag + " info")
    for k in ("reward", "dmin", "dist_to_goal"):
        if k in got:
            np.testing.assert_allclose(got[k], ref[k], atol=atol, rtol=0, err_msg=tag + " " + k)


def oracle_env(params, E, N, S):
    from oracle import oracle
    return oracle.OracleEnv(params, E, N, S)


def oracle_outcome(params, b, act, border=None):
    return robot_outcome_forms(oracle_env, params, b, act, border, forms=("step",))["step"]


def _robot_rows(b, px, py, radius, theta=0.0, goal=None):
    b.robot[:] = 0
    b.robot[:, 0], b.robot[:, 1], b.robot[:, 4], b.robot[:, 7], b.robot[:, 8] = px, py, radius, 1.0, theta
    b.robot[:, 5], b.robot[:, 6] = (FAR_GOAL, FAR_GOAL) if goal is None else goal


# -- 1. tests/golden/collisions.npz: one env per row

def golden_collision_groups():
    """(fixture, {(kinematics, dt): row indices}): dt = 0.25 holds all but the reference's own six unit rows."""
    z = load("collisions")
    groups = {}
    for k in range(len(z["h"])):
        groups.setdefault((int(z["kin"][k]), float(z["dt"][k])), []).append(k)
    return z, {key: np.array(v) for key, v in groups.items()}


def golden_collision_batch(z, rows):
    """n = 1: the human at h with h's velocity and its goal where it stands, type = row index % 3; the robot at r with
    its heading in slot 8 and a far goal -> (batch, the rows' actions)."""
    b = _blank_batch(len(rows), 1, 0)
    h, r = z["h"][rows], z["r"][rows]
    b.px[:, 0], b.py[:, 0], b.vx[:, 0], b.vy[:, 0], b.radius[:, 0] = h.T
    b.gx[:, 0], b.gy[:, 0], b.v_pref[:, 0] = h[:, 0], h[:, 1], 1.0
    b.type[:, 0] = rows % 3
    _robot_rows(b, r[:, 0], r[:, 1], r[:, 3], theta=r[:, 2])
    return b, z["act"][rows]


def check_golden_collisions(make_env, forms=OUTCOME_FORMS):
    """Every row of collisions.npz through every form -> {form: (holonomic rows not bit-identical to the reference,
    holonomic rows, largest |difference| on the unicycle rows)} after the assertions of the issue."""
    z, groups = golden_collision_groups()
    n = len(z["h"])
    typ = np.arange(n) % 3
    got = {}  # form -> (flag [n], min(dmin_in, dmin[type]) [n])
    for (kin, dt), all_rows in sorted(groups.items()):
        params = outcome_params(kin, dt)
        for rows in split_off_wave_multiples(all_rows):
            b, act = golden_collision_batch(z, rows)
            res = robot_outcome_forms(make_env, params, b, act, forms=forms)
            assert_forms_agree(res, "kin %d dt %g" % (kin, dt))
            for form, o in res.items():
                flag, dm = got.setdefault(form, (np.zeros(n, bool), np.zeros(n)))
                t = typ[rows]
                code = np.array(COLLISION_CODE)[t]
                is_code = np.isin(o["info"], COLLISION_CODE)
                assert (is_code <= (o["info"] == code)).all(), "%s: another type's collision code" % form
                flag[rows] = o["info"] == code
                others = np.ones((len(rows), 3), bool)
                others[np.arange(len(rows)), t] = False
                assert np.isinf(o["dmin"][others]).all(), "%s: dmin of a type with no member" % form
                own = o["dmin"][np.arange(len(rows)), t]
                assert np.isinf(own[flag[rows]]).all(), "%s: a colliding row reports a finite dmin" % form
                dm[rows] = np.minimum(z["dmin_in"][rows], own)
    stats = {}
    hol = z["kin"] == _abi.HOLONOMIC
    ref = z["dmin_out"]
    for form, (flag, dm) in got.items():
        np.testing.assert_array_equal(flag, z["coll"], err_msg=form + " collision flag")
        for k in range(int(z["n_unit"])):
            assert bool(flag[k]) == bool(z["unit_expected"][k]), (form, "unit row", k)
        both_inf = np.isinf(dm) & np.isinf(ref) & (dm == ref)
        with np.errstate(invalid="ignore"):
            diff = np.where(both_inf, 0.0, np.abs(dm - ref))
        assert not np.isnan(diff).any() and np.isfinite(diff).all(), form
        not_identical = int((dm[hol] != ref[hol]).sum())
        worst_uni = float(diff[~hol].max())
        print("golden collisions, %-10s %d envs: %d of %d holonomic rows not bit-identical (cap %d), largest holonomic "
              "|diff| %.3g, largest unicycle |diff| %.3g" % (form, n, not_identical, int(hol.sum()),
                                                            int(0.02 * hol.sum()), float(diff[hol].max()), worst_uni))
        assert diff[hol].max() <= 1e-12, (form, "holonomic", float(diff[hol].max()))
        assert not_identical <= 0.02 * hol.sum(), (form, not_identical)
        assert worst_uni <= 1e-9, (form, "unicycle", worst_uni)
        stats[form] = (not_identical, int(hol.sum()), worst_uni)
    return stats


# -- 2. tests/golden/grid.npz: one env per point

def _grid_point_batch(packed, pts):
    """n = 0 (the one human slot unused), the robot at the point with the point's radius, that map as the env's grid."""
    b = _blank_batch(len(pts), 1, 0)
    b.n_humans[:] = 0
    b.grid = np.ascontiguousarray(packed, dtype=np.uint64)
    _robot_rows(b, pts[:, 0], pts[:, 1], pts[:, 2])
    return b


def golden_grid_batches():
    """[(batch, border or None, expected collision)] over all 18 x 400 points of grid.npz: the rows that used the
    fixture's border as calls of their own."""
    z = load("grid")
    packed, pts, exp = [], [], []
    for k in range(int(z["n"])):
        g = pack_grid(1.0 - z["grid_%d" % k])
        packed += [g] * len(z["pts_%d" % k])
        pts.append(z["pts_%d" % k])
        exp.append(z["coll_%d" % k])
    packed, pts, exp = np.stack(packed), np.concatenate(pts), np.concatenate(exp).astype(bool)
    out = []
    for use_border in (False, True):
        for ids in split_off_wave_multiples(np.nonzero(pts[:, 3].astype(bool) == use_border)[0]):
            out.append((_grid_point_batch(packed[ids], pts[ids]), z["border"] if use_border else None, exp[ids]))
    assert sum(b.n for b, _, _ in out) == len(pts) and float(z["map_size_m"]) == 9.0 and float(z["map_resolution"]) == 0.1
    return out


def check_obstacle_outcome(make_env, params, b, border, expected, tag, forms=OUTCOME_FORMS):
    """Standing robots with no human: info is INFO_COLLISION_OBSTACLE (terminal) exactly where expected, else a
    non-terminal INFO_NOTHING, in every form, and the forms agree byte for byte."""
    res = robot_outcome_forms(make_env, params, b, np.zeros((b.n, 2)), border, forms)
    assert_forms_agree(res, tag)
    want = np.where(expected, _abi.INFO_COLLISION_OBSTACLE, _abi.INFO_NOTHING)
    for form, o in res.items():
        bad = np.nonzero(o["info"] != want)[0]
        assert not len(bad), "%s %s: %d of %d envs, the first %d: info %d, expected %d" % (
            tag, form, len(bad), b.n, bad[0], o["info"][bad[0]], want[bad[0]])
        np.testing.assert_array_equal(o["done"].astype(bool), expected, err_msg=tag + " " + form)
    return res


# -- 3. grid windows the goldens do not reach

def grid_window_restated(occ, map_size_m, map_resolution, px, py, radius, border=None):
    """simulator/env.py:227-271 in plain Python / numpy: indices rounded half to even, the clipped slice, .any()."""
    lim = int(round(map_size_m / map_resolution))
    ix = int(round((px + map_size_m / 2.0) / map_resolution))
    iy = int(round((py + map_size_m / 2.0) / map_resolution))
    h = int(np.ceil(radius / np.sqrt(2.0) / map_resolution))
    sx, ex = max(ix - h, 0), min(ix - h + 2 * h, lim)
    sy, ey = max(iy - h, 0), min(iy - h + 2 * h, lim)
    hit = False
    if ex > sx and ey > sy:
        hit = bool(occ[sx:ex, sy:ey].any())
    if border is not None:
        hit = hit or bool(px <= border[0] + radius or px >= border[1] - radius or py <= border[2] + radius
                          or py >= border[3] - radius)
    return hit


GRID_MAPS = ((9.0, 0.1), (9.0, 0.075), (12.8, 0.1))  # G = 90, 120, 128
GRID_RADII = (0.6, 0.9, 1.5)  # windows of 10, 14 and 22 rows at 0.1 m: the row loop after the eight unrolled rows runs
GRID_BORDER = (-3.0, 3.0, -2.5, 3.5)
WIDE_RADIUS = 9.0  # ceil(9 / sqrt(2) / 0.1) = 64: from index 64 the window spans all 128 columns of a G = 128 map


def grid_window_cases(map_size_m, res):
    """[(occupied [G, G] bool, px, py, radius, border or None, note)] for one map geometry."""
    G = int(round(map_size_m / res))
    half = map_size_m / 2.0
    cases = []

    def cell_map(cells):
        occ = np.zeros((G, G), bool)
        for x, y in cells:
            if 0 <= x < G and 0 <= y < G:
                occ[x, y] = True
        return occ

    def at(i, frac=0.0):  # the coordinate of index i (+ frac cells: 0.5 is the half-cell boundary)
        return (i + frac) * res - half
    for radius in GRID_RADII:
        h = int(np.ceil(radius / np.sqrt(2.0) / res))
        mid = G // 2
        # a single occupied cell at the first / last column (row) of the window and one outside it on each side
        targets = [(mid, c) for c in (0, 63, 64, G - 1)] + [(r, mid) for r in (0, G - 1)]
        for (r, c) in targets:
            occ = cell_map([(r, c)])
            for off in (-h, -h + 1, h, h + 1):
                for frac in (0.0, 0.5, -0.5):
                    cases.append((occ, at(r), at(c + off, frac), radius, None, "cell (%d, %d) column offset %d" % (r, c, off)))
                    cases.append((occ, at(r + off, frac), at(c), radius, None, "cell (%d, %d) row offset %d" % (r, c, off)))
        # the only occupied cells lie one column / row outside the window on each side; and just inside it
        for ci in (mid, h, G - h):
            lo, hi = ci - h, ci + h  # the window is [lo, hi)
            ring = [(ci, lo - 1), (ci, hi), (lo - 1, ci), (hi, ci), (lo - 1, lo - 1), (hi, hi)]
            cases.append((cell_map(ring), at(ci), at(ci), radius, None, "cells one outside the window"))
            for cell in ((ci, lo), (ci, hi - 1), (lo, ci), (hi - 1, ci)):
                cases.append((cell_map([cell]), at(ci), at(ci), radius, None, "cell on the window's edge"))
        # the four corners and points up to a radius outside the map, on a map with every cell occupied and on one with
        # the four corner cells: the window clips to a sliver, then to nothing
        corners = cell_map([(0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1)])
        full = np.ones((G, G), bool)
        for sx in (-1, 1):
            for sy in (-1, 1):
                for out in (0.0, 0.25, 0.5, 0.75, 1.0, 1.25):
                    for occ in (corners, full):
                        cases.append((occ, sx * (half + out * radius), sy * half, radius, None, "outside in x"))
                        cases.append((occ, sx * half, sy * (half + out * radius), radius, None, "outside in y"))
                        cases.append((occ, sx * (half + out * radius), sy * (half + out * radius), radius, None, "outside in both"))
    # the border's four equalities (<= / >=: a collision) and one ulp inside each (none), on an empty map
    empty = np.zeros((G, G), bool)
    r, bd = 1.5, GRID_BORDER
    for px, py, inward in ((bd[0] + r, 0.5, (1, 0)), (bd[1] - r, 0.5, (-1, 0)), (0.0, bd[2] + r, (0, 1)), (0.0, bd[3] - r, (0, -1))):
        cases.append((empty, px, py, r, bd, "border equality"))
        cases.append((empty, float(np.nextafter(px, px + inward[0])) if inward[0] else px,
                      float(np.nextafter(py, py + inward[1])) if inward[1] else py, r, bd, "one ulp inside the border"))
    cases.append((empty, 0.0, 0.5, r, bd, "well inside the border"))
    if G == 128:  # the window over all 128 columns, and over 127 and 126 of them
        for iy in (64, 65, 63, 62):
            for cell in ((5, 127), (5, 0), (5, 64), (5, 63), (127, 126), None):
                occ = cell_map([cell] if cell else [])
                cases.append((occ, at(64), at(iy), WIDE_RADIUS, None, "wide window at column index %d" % iy))
    return cases


def grid_window_batches(map_size_m, res):
    """[(batch, border, expected from the restatement, notes)] of a geometry: the border cases as a call of their own."""
    cases = grid_window_cases(map_size_m, res)
    out = []
    for with_border in (False, True):
        sel = [c for c in cases if (c[4] is not None) == with_border]
        while len(sel) % 4 == 0:
            sel.append(sel[len(sel) // 3])
        pts = np.array([[c[1], c[2], c[3]] for c in sel])
        b = _grid_point_batch(np.stack([pack_grid(1.0 - c[0].astype(np.float64)) for c in sel]), pts)
        border = GRID_BORDER if with_border else None
        exp = np.array([grid_window_restated(c[0], map_size_m, res, c[1], c[2], c[3], border) for c in sel])
        out.append((b, border, exp, [c[5] for c in sel], [c[0] for c in sel]))
    return out


# -- 4. the ordered per-type reduction: standing humans at exact gaps around a standing robot

ORDERED_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 17, 24, 25, 32, 33)
ORDERED_ENVS = 203  # 7 * 29: no multiple of 4 lanes per env, 16 envs per wave or 64
ROBOT_RADIUS = 0.25
COLLIDER = -1.0 / 16


def place_standing(b, e, i, gap, origin=(0.0, 0.0)):
    """Human i of env e stands still on axis i % 4, radius 0.25 + (i // 4) / 8, its boundary `gap` from the robot's
    (radius 0.25 at `origin`): all binary fractions, so the reference distance is exactly `gap`."""
    rad = 0.25 + (i // 4) * 0.125
    d = ROBOT_RADIUS + rad + gap
    ax, ay = ((1, 0), (0, 1), (-1, 0), (0, -1))[i % 4]
    b.px[e, i], b.py[e, i] = origin[0] + ax * d, origin[1] + ay * d
    b.gx[e, i], b.gy[e, i] = b.px[e, i], b.py[e, i]
    b.vx[e, i] = b.vy[e, i] = 0.0
    b.radius[e, i], b.v_pref[e, i] = rad, 1.0


def _distinct_gaps(gap, n):
    """Two humans on one axis must not stand on one spot (ORCA's coincident twins are not this test's business): a
    non-collider that would is moved out by 1/64 until it does not."""
    for i in range(n):
        def spot(j):
            return 0.25 + (j // 4) * 0.125 + gap[j]
        while gap[i] >= 0 and any(spot(j) == spot(i) for j in range(i % 4, n, 4) if j != i):
            gap[i] = gap[i] + 1.0 / 64 if gap[i] < 63.0 / 64 else 1.0 / 64
    return gap


def ordered_batch(N, interleaved):
    """ORDERED_ENVS envs of up to N standing humans (b.gap [E, N] holds the exact distances): hand-built envs for the
    order-dependent cases first, a seeded random fill after them.  Types are grouped as SceneBatch.from_scenes lays
    them out, or, with `interleaved`, mixed by index."""
    rs = np.random.RandomState(9100 + 2 * N + int(interleaved))
    E = ORDERED_ENVS
    b = _blank_batch(E, N, 0)
    _robot_rows(b, 0.0, 0.0, ROBOT_RADIUS)
    gap = np.full((E, N), 0.5)
    typ = np.zeros((E, N), np.uint8)
    n_h = np.full(E, N, np.int32)
    c = -(-N // 4)  # the humans of one quarter
    e = 0
    n_h[e] = 0  # an empty env
    e += 1
    if N >= 5:
        for t in range(3):
            for q in range(4):
                fi = q * c  # the first collider of type t opens quarter q
                if fi >= N:
                    continue
                typ[e] = [(t + 1 + i % 2) % 3 for i in range(N)] if interleaved else t
                keys = [0, fi] + [i for i in (fi + 1, fi + 2) if i < N]
                typ[e, keys] = t
                gap[e, fi] = COLLIDER
                if q > 0:
                    gap[e, 0] = 8.0 / 64  # the closest of its type, a quarter earlier: counts
                if fi + 1 < N:
                    gap[e, fi + 1] = 1.0 / 64  # closer still, behind the collider: ignored
                if fi + 2 < N:
                    gap[e, fi + 2] = COLLIDER  # a second collider behind the first
                e += 1
        for hit in ((0, 1), (0, 2), (1, 2), (0, 1, 2)):  # two and three types collide in one env
            typ[e] = np.arange(N) % 3 if interleaved else np.sort(np.arange(N) % 3)
            for t in hit:
                gap[e, int(np.argmax(typ[e] == t))] = COLLIDER
            e += 1
    while e < E:
        n_h[e] = N - rs.randint(0, min(N, 3) + 1)  # ragged: n in [N - 3, N]
        kinds = rs.choice(3, size=rs.randint(1, 4), replace=False)  # one to three types present
        typ[e] = rs.choice(kinds, size=N)
        if not interleaved:
            typ[e] = np.sort(typ[e])
        p_hit = rs.choice([0.0, 0.1, 0.3])
        gap[e] = np.where(rs.uniform(size=N) < p_hit, COLLIDER, rs.randint(1, 64, size=N) / 64.0)
        e += 1
    for e in range(E):
        _distinct_gaps(gap[e], int(n_h[e]))
        for i in range(N):
            place_standing(b, e, i, gap[e, i])
    b.n_humans[:], b.type[:] = n_h, typ
    _clear_unused(b)
    b.gap = gap
    return b


def ordered_walk_restated(b):
    """simulator/env.py:303-313 per type over the exact gaps -> (dmin [E, 3], collision [E, 3]) and, for the coverage,
    what[e][t] = dict(first collider's index, quarter, closer_behind, closer_before_earlier_quarter, second_collider)."""
    E, N = b.n, b.N
    c = -(-N // 4)
    dmin = np.full((E, 3), np.inf)
    coll = np.zeros((E, 3), bool)
    what = [[None] * 3 for _ in range(E)]
    for e in range(E):
        n = int(b.n_humans[e])
        for t in range(3):
            members = [i for i in range(n) if b.type[e, i] == t]
            best = None
            for i in members:
                if b.gap[e, i] < 0:
                    coll[e, t] = True
                    behind = [j for j in members if j > i]
                    what[e][t] = dict(first=i, quarter=i // c,
                                      closer_behind=any(0 <= b.gap[e, j] < dmin[e, t] for j in behind),
                                      closer_before_earlier_quarter=best is not None and best // c < i // c,
                                      second_collider=any(b.gap[e, j] < 0 for j in behind))
                    break
                if b.gap[e, i] < dmin[e, t]:
                    dmin[e, t] = b.gap[e, i]
                    best = i
    return dmin, coll, what


def ordered_coverage(b):
    """The order-dependent cases a batch holds, counted from the restatement alone."""
    dmin, coll, what = ordered_walk_restated(b)
    cov = {}
    for t in range(3):
        for q in range(4):
            cov["type %d first collider in quarter %d" % (t, q)] = sum(1 for w in what if w[t] and w[t]["quarter"] == q)
        for k in ("closer_behind", "closer_before_earlier_quarter", "second_collider"):
            cov["type %d %s" % (t, k)] = sum(1 for w in what if w[t] and w[t][k])
        cov["type %d without a member" % t] = int(((b.type != t) | (np.arange(b.N)[None] >= b.n_humans[:, None])).all(1).sum())
    cov["two types collide"] = int((coll.sum(1) == 2).sum())
    cov["three types collide"] = int((coll.sum(1) == 3).sum())
    cov["humans but no collider"] = int(((coll.sum(1) == 0) & (b.n_humans > 0)).sum())
    cov["empty env"] = int((b.n_humans == 0).sum())
    return cov


def check_ordered(make_env, N, interleaved, forms=OUTCOME_FORMS):
    """dmin of every form bitwise the restatement's and the oracle's; info / done the oracle's; the forms byte-identical."""
    b = ordered_batch(N, interleaved)
    params = outcome_params()
    act = np.zeros((b.n, 2))
    dmin, coll, _ = ordered_walk_restated(b)
    ref = oracle_outcome(params, b, act)
    tag = "N %d %s" % (N, "interleaved" if interleaved else "grouped")
    np.testing.assert_array_equal(ref["dmin"], dmin, err_msg=tag + ": the oracle against the restatement")
    res = robot_outcome_forms(make_env, params, b, act, forms=forms)
    for form, o in res.items():
        bad = np.argwhere(o["dmin"] != dmin)
        assert not len(bad), "%s %s: dmin of %d (env, type), the first %s: %r, expected %r (n = %d, types %s, gaps %s)" % (
            tag, form, len(bad), bad[0].tolist(), o["dmin"][tuple(bad[0])], dmin[tuple(bad[0])], b.n_humans[bad[0][0]],
            b.type[bad[0][0]].tolist(), b.gap[bad[0][0]].tolist())
        assert_outcome(o, ref, tag + " " + form)
    assert_forms_agree(res, tag)
    return b, res


# -- 5. the reward ladder

LADDER = dict(collision_penalty=(-0.25, -0.5, -0.75, -0.125), discomfort_dist=(0.125, 0.25, 0.375),
              discomfort_factor=(0.5, 1.0, 2.0), success_reward=1.0, max_goal_distance=16.0, time_good=10.0,
              time_max=20.0)
LADDER_BORDER = (-4.0, 4.0, -4.0, 4.0)


def ladder_params(new_reward, time_limit=25.0, **kw):
    args = dict(LADDER, new_reward=new_reward, time_limit=time_limit)
    args.update(kw)
    return outcome_params(**args)


def ladder_batch(wall):
    """One standing human per type around a standing robot: colliding subset of {adult, bicycle, child, wall} (16) x
    goal reached or not (2) x which humans stand inside their type's discomfort distance (8), then the exact
    thresholds.  wall = "grid": the wall is an occupied cell under the robot; "border": the robot stands where
    px == border[0] + radius under LADDER_BORDER (pass it to the call).  b.meta[e] = (colliding subset, reached, inside)."""
    dd = LADDER["discomfort_dist"]
    rows = [(sub, reached, inside) for sub in range(16) for reached in (0, 1) for inside in range(8)]
    extra = [("goal at the radius", None), ("goal one ulp inside", None)]
    extra += [("gap == discomfort_dist", t) for t in range(3)] + [("gap 1/64 under discomfort_dist", t) for t in range(3)]
    extra += [("gap 0", t) for t in range(3)]
    E = len(rows) + len(extra)
    assert E % 4
    G = 90
    b = _blank_batch(E, 3, 0)
    b.grid = np.zeros((E, G, 2), np.uint64)
    b.type[:] = (0, 1, 2)
    meta = []
    under_robot = pack_grid(1.0 - (np.arange(G)[:, None] == 45) * (np.arange(G)[None] == 45) * 1.0)
    for e in range(E):
        origin, goal_dx, gaps = (0.0, 0.0), 3.0, [0.5, 0.5, 0.5]
        if e < len(rows):
            sub, reached, inside = rows[e]
            for t in range(3):
                gaps[t] = COLLIDER if sub >> t & 1 else (dd[t] / 2 if inside >> t & 1 else 0.5)
            if sub >> 3 & 1:
                if wall == "grid":
                    b.grid[e] = under_robot
                else:
                    origin = (LADDER_BORDER[0] + ROBOT_RADIUS, 0.0)
            goal_dx = 0.125 if reached else 3.0
            meta.append((sub, reached, inside))
        else:
            name, t = extra[e - len(rows)]
            if name == "goal at the radius":
                goal_dx = ROBOT_RADIUS
            elif name == "goal one ulp inside":
                goal_dx = float(np.nextafter(ROBOT_RADIUS, 0.0))
            elif name == "gap == discomfort_dist":
                gaps[t] = dd[t]
            elif name == "gap 1/64 under discomfort_dist":
                gaps[t] = dd[t] - 1.0 / 64
            else:
                gaps[t] = 0.0
            meta.append(name)
        b.robot[e] = [origin[0], origin[1], 0.0, 0.0, ROBOT_RADIUS, origin[0] + goal_dx, origin[1], 1.0, 0.0]
        for t in range(3):
            place_standing(b, e, t, gaps[t], origin)
    b.meta = meta
    return b


def unicycle_batch():
    """A standing unicycle robot (v = 0) that turns by a1 = 0, 0.5 or -0.5, with no human or one of each type inside its
    discomfort distance: 9 envs; run under rotation_penalty_factor 0 and 0.5."""
    cases = [(a1, t) for a1 in (0.0, 0.5) for t in (None, 0, 1, 2)] + [(-0.5, None)]
    b = _blank_batch(len(cases), 3, 0)
    b.type[:] = (0, 1, 2)
    _robot_rows(b, 0.0, 0.0, ROBOT_RADIUS, theta=np.pi / 2)
    for e, (a1, t) in enumerate(cases):
        for k in range(3):
            place_standing(b, e, k, LADDER["discomfort_dist"][k] / 2 if k == t else 0.5)
    return b, np.array([[0.0, a1] for a1, _ in cases])


TIME_REWARD = dict(time_good=0.5, time_max=1.0)
TIME_STEPS = 9
ARRIVALS = (0.0, 0.25, 0.5, 0.75, 1.0, 1.25, None)


def time_reward_batch():
    """ROBOT_LINEAR robots (v_pref 1, radius 0.25, dt 0.25) whose goals lie 0.375 + t ahead: they arrive in the step that
    starts at t = 0, 0.25, ... 1.25; the last one never does and times out at t == time_limit = 2."""
    b = _blank_batch(len(ARRIVALS), 1, 0)
    b.n_humans[:] = 0
    _robot_rows(b, 0.0, 0.0, ROBOT_RADIUS)
    for e, t in enumerate(ARRIVALS):
        b.robot[e, 5:7] = (FAR_GOAL if t is None else 0.375 + t, 0.0)
    return b, ladder_params(1, time_limit=2.0, **TIME_REWARD)


def time_reward_forms(make_env, forms=("step", "orca", "one_launch")):
    """TIME_STEPS steps of time_reward_batch under ROBOT_LINEAR -> {form: {key: [K, E]}} (the look-ahead takes supplied
    actions only and has no part in this one)."""
    b, params = time_reward_batch()
    res = {}
    for form in forms:
        env = make_env(params, b.n, b.N, b.S)
        env.reset(b)
        if form == "one_launch":
            o = env.step_k(TIME_STEPS, OUTCOME_KEYS, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR,
                           flags=_abi.FLAG_ONE_LAUNCH)
        else:
            pol = _abi.HUMAN_LINEAR if form == "step" else _abi.HUMAN_ORCA
            outs = [env.step(human_policy=pol, robot_policy=_abi.ROBOT_LINEAR) for _ in range(TIME_STEPS)]
            o = {k: np.stack([s[k] for s in outs]) for k in OUTCOME_KEYS}
        res[form] = {k: np.array(o[k]) for k in OUTCOME_KEYS}
        _close(env)
    return res


def check_against_oracle(make_env, params, b, act, border, tag, forms=OUTCOME_FORMS):
    """Every form at the bars of assert_outcome against the oracle's step, and byte for byte against each other."""
    ref = oracle_outcome(params, b, act, border)
    res = robot_outcome_forms(make_env, params, b, act, border, forms)
    for form, o in res.items():
        assert_outcome(o, ref, tag + " " + form)
    assert_forms_agree(res, tag)
    return ref, res
