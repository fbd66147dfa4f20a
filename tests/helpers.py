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
               "traj_unicycle_rotpen"]
TRAJ_ORCASUB = ["traj_a5_linear_orcasub", "traj_a5_scripted_orcasub",
                "traj_a3b3s2_scripted_orcasub", "traj_n10_walls_t17_orcasub"]
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
# name -> (maxNeighbors, neighborDist)
ORCA_PARAM_SETS = {"default": (10, 10.0), "mn3-nd2": (3, 2.0), "mn1": (1, 10.0), "mn0": (0, 10.0)}
ORCA_HUMAN_CASES = ([(n, rv, ps) for n, rv in ORCA_HUMAN_COUNTS for ps in ("default", "mn3-nd2")]
                    + [(n, 0, ps) for n in (6, 13) for ps in ("mn1", "mn0")])
# (humans, static rows) of the robot's own ORCA: rows 1..13, 16, 17, 21, 22, 32
ORCA_ROBOT_CASES = [(r, 0) for r in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 22)] + [(6, 4), (10, 11), (20, 12)]
ORCA_STEPS = 3


def orca_case_id(case):
    return "N%d%s-%s" % (case[0], "+robot" if case[1] else "", case[2]) if len(case) == 3 else "N%d-S%d" % case


def orca_case_params(rv=0, param_set="default"):
    params = params_of(load("traj_n10_walls_t17_orcasub"))  # time_step 0.25, horizon 5
    params.robot_visible = rv
    params.orca_max_neighbors, params.orca_neighbor_dist = ORCA_PARAM_SETS[param_set]
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
    from oracle import oracle
    N, S = case
    b = orca_robot_batch(N, S)
    o = oracle.OracleEnv(orca_case_params(), b.n, N, S, library=library)
    o.reset(b)
    return o.robot_orca(safety)
