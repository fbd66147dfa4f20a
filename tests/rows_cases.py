"""The rotated observation rows held to the float32 rule bit for bit: the rule, the probe scenes, the forms and the
look-ahead's shape table.  tests/test_rotated_rows_cpu.py proves the method on the oracle, tests/test_rotated_rows_gpu.py
holds the seven sites of the device to it.

The method.  rot_frame / rotate_row (csrc/ebc_device.h, the restatement of rl/policy/cadrl.py:236-337) are float32
`+ - * sqrt` on cast inputs, but for three calls: rot = atan2f(dy, dx), c = cosf(rot), s = sinf(rot), and those are not
the same function in glibc and in the device's library.  A PROBE ROW takes them out of the comparison: a row whose
velocity is exactly (1, 0) comes out with out[8] = 1 * c + 0 * s = c and out[9] = 0 * c - 1 * s = -s, both exact, so
every frame reports its own c and s, and every other value of every row of that frame is a fixed sequence of float32
operations on known inputs, which numpy float32 reproduces in every bit (rule_rows).  What is left of the frame — c and s
themselves and, under rotate_unicycle, column 2 = float32(theta) - rot — is held to float64 within a bar measured on
the oracle (frame_error).

No GPU and no torch at module level."""
import numpy as np

from ebcsim import _abi
from ebcsim.scene import SceneBatch
from helpers import _close, load, params_of

F = np.float32
LA_THREADS = 256  # EBC_LA_THREADS: rows per chunk of the look-ahead's phase C


# ---- the rule ---------------------------------------------------------------------------------------------------------

def rule_rows(robot9, rows5, types, T, unicycle, c, s, rot=None, n_rows=None):
    """rot_frame + rotate_row in numpy float32 -> float32 [..., R, T].  robot9 [..., 9] and rows5 [..., R, 5] are doubles,
    cast once; every product and every sum is an operation of its own (numpy fuses nothing).  c, s [...]: the frame's
    cosine and sine (frame_of).  Column 2 is float32(theta) - rot under rotate_unicycle (`rot` [...] float32; without
    it the column is NaN: the caller leaves it out), else +0.  Columns 13..16 (T = 17) are the one-hot of the type.
    Rows at or past n_rows [...] (default: none) are +0 in every bit."""
    rb = np.asarray(robot9, np.float64).astype(F)[..., None, :]
    rw = np.asarray(rows5, np.float64).astype(F)
    types = np.asarray(types)
    c = np.asarray(c, F)[..., None]
    s = np.asarray(s, F)[..., None]
    px, py, vx, vy, r, gx, gy, vpref, theta = (rb[..., k] for k in range(9))
    px1, py1, vx1, vy1, r1 = (rw[..., k] for k in range(5))
    out = np.zeros(rw.shape[:-1] + (T,), F)
    dx, dy = gx - px, gy - py
    out[..., 0] = np.sqrt(dx * dx + dy * dy)
    out[..., 1] = vpref
    if unicycle:
        out[..., 2] = F(np.nan) if rot is None else theta - np.asarray(rot, F)[..., None]
    out[..., 3] = r
    out[..., 4] = vx * c + vy * s
    out[..., 5] = vy * c - vx * s
    out[..., 6] = (px1 - px) * c + (py1 - py) * s
    out[..., 7] = (py1 - py) * c - (px1 - px) * s
    out[..., 8] = vx1 * c + vy1 * s
    out[..., 9] = vy1 * c - vx1 * s
    out[..., 10] = r1
    ex, ey = px - px1, py - py1
    out[..., 11] = np.sqrt(ex * ex + ey * ey)
    out[..., 12] = r + r1
    if T == 17:
        for k in range(4):
            out[..., 13 + k] = (types == k).astype(F)
    assert out.dtype == F
    if n_rows is not None:
        pad = np.arange(rw.shape[-2]) >= np.asarray(n_rows)[..., None]
        out[pad] = 0
    return out


def frame_of(rows):
    """(c, s) of the frame(s) from the probe row 0: rows [..., R, T] -> two float32 [...]."""
    rows = np.asarray(rows)
    return rows[..., 0, 8].copy(), -rows[..., 0, 9]


def frame_error(robot9, c, s, col2=None):
    """The frame against float64: theta = atan2 of the float32 (dy, dx) in float64 -> (max |c - cos theta|,
    max |s - sin theta|, max |col2 - (float32(theta_robot) - theta)| or 0 without col2)."""
    rb = np.asarray(robot9, np.float64).astype(F)
    dx, dy = (rb[..., 5] - rb[..., 0]).astype(np.float64), (rb[..., 6] - rb[..., 1]).astype(np.float64)
    th = np.arctan2(dy, dx)
    ec = float(np.abs(np.asarray(c, np.float64) - np.cos(th)).max())
    es = float(np.abs(np.asarray(s, np.float64) - np.sin(th)).max())
    e2 = 0.0
    if col2 is not None:
        e2 = float(np.abs(np.asarray(col2, np.float64) - (rb[..., 8].astype(np.float64) - th)).max())
    return ec, es, e2


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_rows_equal_rule(rec, T, unicycle, tag, rot=None, select=None):
    """Every bit (the sign of zero included) of a record's rotated rows against rule_rows with the frame the record's own
    probe row reports; padding rows +0.  Without `rot`, column 2 is left out under rotate_unicycle.  select [...]: the
    frames compared (default all).  -> rows compared."""
    got = rec["rot"]
    c, s = frame_of(got)
    assert np.isfinite(c).all() and np.isfinite(s).all(), tag
    # the probe itself: raw velocity exactly (1, 0), or the frame is not what columns 8 and 9 report
    raw = np.broadcast_to(rec["raw"], got.shape[:-1] + (5,))
    assert (raw[..., 0, 2] == 1.0).all() and (raw[..., 0, 3] == 0.0).all(), tag + ": the probe's velocity is not (1, 0)"
    n_rows = np.broadcast_to(rec["n_rows"], got.shape[:-2])
    want = rule_rows(rec["robot"], raw, np.broadcast_to(rec["types"], got.shape[:-1]), T, unicycle, c, s, rot, n_rows)
    if unicycle and rot is None:  # column 2 of the rows that exist is the frame's business (frame_error)
        want[..., 2] = np.where(np.arange(got.shape[-2]) < n_rows[..., None], got[..., 2], F(0))
    differ = bits(got) != bits(want)
    if select is not None:
        differ &= np.broadcast_to(select, got.shape[:-2])[..., None, None]
    bad = np.argwhere(differ)
    assert not len(bad), "%s: %d values differ from the rule, the first at %s: %r, the rule %r" % (
        tag, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    frames = got.shape[:-2] if select is None else (int(np.broadcast_to(select, got.shape[:-2]).sum()),)
    return int(np.prod(frames)) * got.shape[-2]


# ---- the probe --------------------------------------------------------------------------------------------------------

PROBE_X = (9.0, 10.0)  # the probe stands here: 5 m and more from the box [-4, 4]^2 that holds every other agent, static
#                        row and goal, and walks away from it — with orca_neighbor_dist 2 it never has an ORCA line


def rows_params(T, unicycle):
    """time_step 0.25; the robot invisible and ORCA's neighbour range 2 m, so that the probe human has no neighbour."""
    p = params_of(load("traj_n10_walls_t17_orcasub"))
    p.with_agent_type = int(T == 17)
    p.robot_kinematics = _abi.UNICYCLE if unicycle else _abi.HOLONOMIC
    p.rotate_unicycle = int(bool(unicycle))
    p.robot_visible = 0
    p.orca_neighbor_dist = 2.0
    p.time_limit = 100.0
    assert _abi.rot_width(p) == T
    return p


def probe_batch(rs, E, N, S, theta=None):
    """Synthetic scenes in the style of test_gpu_parity._synthetic_batch: ragged n_humans >= 1 (env 0 full, env 1 one
    human and no static row, env 2 every human and no static row), ragged static rows, uniform doubles (none
    float32-representable).  Human 0 of every env is the probe under every human policy: velocity exactly (1, 0), its
    goal due +x (gy = py, gx = px + 30), v_pref 1, out of everyone's range (PROBE_X).  theta: the robot's heading
    (default random)."""
    n = rs.randint(1, N + 1, size=E).astype(np.int32)
    ns = rs.randint(0, S + 1, size=E).astype(np.int32) if S else np.zeros(E, np.int32)
    n[0], ns[0] = N, S
    if E > 1:
        n[1], ns[1] = 1, 0
    if E > 2:
        n[2], ns[2] = N, 0
    f = lambda *sh: np.zeros(sh)  # noqa: E731
    b = SceneBatch(E, N, S, n, f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N), f(E, N),
                   np.zeros((E, N), np.uint8), ns, f(E, max(S, 1)), f(E, max(S, 1)), f(E, max(S, 1)), None, f(E, 9))
    for e in range(E):
        k = n[e]
        b.px[e, :k], b.py[e, :k] = rs.uniform(-4, 4, k), rs.uniform(-4, 4, k)
        b.vx[e, :k], b.vy[e, :k] = rs.uniform(-0.5, 0.5, k), rs.uniform(-0.5, 0.5, k)
        b.gx[e, :k], b.gy[e, :k] = rs.uniform(-4, 4, k), rs.uniform(-4, 4, k)
        b.radius[e, :k], b.v_pref[e, :k] = rs.uniform(0.1, 0.5, k), rs.uniform(0.3, 1.2, k)
        b.type[e, :k] = np.sort(rs.randint(0, 3, k))
        m = ns[e]
        b.spx[e, :m], b.spy[e, :m] = rs.uniform(-4, 4, m), rs.uniform(-4, 4, m)
        b.sradius[e, :m] = rs.uniform(0.3, 0.8, m)
        b.robot[e] = [rs.uniform(-1, 1), rs.uniform(-3.5, -2.5), rs.uniform(-0.5, 0.5), rs.uniform(-0.5, 0.5),
                      rs.uniform(0.2, 0.4), rs.uniform(-0.5, 0.5), rs.uniform(2.5, 3.5), rs.uniform(0.6, 0.9),
                      rs.uniform(0.1, 3.0) if theta is None else theta]
        b.px[e, 0], b.py[e, 0] = rs.uniform(*PROBE_X), rs.uniform(-4, 4)
        b.vx[e, 0], b.vy[e, 0] = 1.0, 0.0
        b.gx[e, 0], b.gy[e, 0], b.v_pref[e, 0] = b.px[e, 0] + 30.0, b.py[e, 0], 1.0
    return b


def place(b, src, dst):
    """Env `dst` of the batch becomes a copy of env `src`."""
    for k in ("n_humans", "px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type", "n_static", "spx", "spy",
              "sradius", "robot"):
        getattr(b, k)[dst] = getattr(b, k)[src]
    return b


def row_types(b):
    """types [E, R] and rows that exist [E] of a batch (no restart changes them in these tests)."""
    R = b.N + b.S
    t = np.zeros((b.n, R), np.int64)
    t[:, :b.N] = b.type
    for e in range(b.n):
        t[e, b.n_humans[e]:] = _abi.ADULT_STATIC
    return t, b.n_humans.astype(np.int64) + (b.n_static.astype(np.int64) if b.S else 0)


def robot_actions(K, E, unicycle, seed=11):
    """[K, E, 2] supplied robot actions: holonomic velocities in +-0.7, or (speed, rotation) under unicycle."""
    rs = np.random.RandomState(seed)
    if unicycle:
        return np.stack([rs.uniform(0.0, 0.7, (K, E)), rs.uniform(-0.5, 0.5, (K, E))], -1)
    return rs.uniform(-0.7, 0.7, (K, E, 2))


def external_actions(b, seed=12):
    """[E, N, 2] supplied human velocities for HUMAN_EXTERNAL: the probe's is (1, 0), unused humans 0."""
    rs = np.random.RandomState(seed)
    act = rs.uniform(-0.5, 0.5, (b.n, b.N, 2))
    act[:, 0] = (1.0, 0.0)
    for e in range(b.n):
        act[e, b.n_humans[e]:] = 0
    return act


def la_actions(A, unicycle, seed=13):
    """[A, 2] look-ahead actions (random doubles, not an action space: any A); under unicycle every third rotation,
    the first included, is exactly 0."""
    rs = np.random.RandomState(seed + A)
    if not unicycle:
        return rs.uniform(-0.7, 0.7, (A, 2))
    act = np.stack([rs.uniform(0.0, 0.7, A), rs.uniform(-0.7, 0.7, A)], -1)
    act[::3, 1] = 0.0
    return act


def propagate(robot, actions, unicycle, dt):
    """CADRL.propagate of the robot for every action (rl/policy/cadrl.py:118-165): [E, 9], [A, 2] -> [E, A, 9] in plain
    doubles.  Under unicycle cos and sin are the host's: exact (hence the device's) only for next heading 0."""
    robot, actions = np.asarray(robot, np.float64), np.asarray(actions, np.float64)
    nb = np.repeat(robot[:, None, :], len(actions), 1)
    a0, a1 = actions[None, :, 0], actions[None, :, 1]
    if not unicycle:
        nb[..., 0] = robot[:, None, 0] + a0 * dt
        nb[..., 1] = robot[:, None, 1] + a1 * dt
        nb[..., 2], nb[..., 3] = a0, a1
    else:
        nth = robot[:, None, 8] + a1
        nvx, nvy = a0 * np.cos(nth), a0 * np.sin(nth)
        nb[..., 0] = robot[:, None, 0] + nvx * dt
        nb[..., 1] = robot[:, None, 1] + nvy * dt
        nb[..., 2], nb[..., 3], nb[..., 8] = nvx, nvy, nth
    return nb


# ---- the forms: (make_env, params, batch, ...) -> records -------------------------------------------------------------
# A record is what one call returned for one set of frames: robot [..., 9] the states the frames were built from,
# raw [..., R, 5] the world-frame rows, rot [..., R, T] the rotated rows, types [..., R], n_rows [...], and `site`, the
# name of the code site that wrote rot.  The leading shape is [E], for the look-ahead [E, A] (raw, types and n_rows
# [E, 1, ...]: they broadcast over the actions).

STEPS = 3
POLICY_NAME = {_abi.HUMAN_EXTERNAL: "external", _abi.HUMAN_LINEAR: "linear", _abi.HUMAN_ORCA: "orca"}


def _rec(site, b, robot, raw, rot, **extra):
    types, n_rows = row_types(b)
    r = dict(site=site, robot=np.array(robot), raw=np.array(raw), rot=np.array(rot), types=types, n_rows=n_rows)
    r.update(extra)
    return r


def _unicycle(params):
    return params.robot_kinematics != _abi.HOLONOMIC


def _step(env, b, act, policy):
    if policy == _abi.HUMAN_EXTERNAL:
        env.set_human_actions(external_actions(b))
    return env.step(robot_action=act, human_policy=policy)


def form_observe(make_env, params, b):
    """ebc_observe at reset and after each of STEPS steps (HUMAN_LINEAR); the robot state from get_state."""
    env = make_env(params, b.n, b.N, b.S)
    env.reset(b)
    acts = robot_actions(STEPS, b.n, _unicycle(params))
    recs, last = [], None
    for t in range(STEPS + 1):
        ob, rot = env.observe()
        recs.append(_rec("observe_kernel", b, env.get_state()["robot"], ob, rot, step=t, returned=last))
        if t < STEPS:
            last = _step(env, b, acts[t], _abi.HUMAN_LINEAR)
    _close(env)
    return recs


def _form_step(make_env, params, b, policies, site):
    env = make_env(params, b.n, b.N, b.S)
    acts = robot_actions(STEPS, b.n, _unicycle(params))
    recs = []
    for policy in policies:
        env.reset(b)
        for t in range(STEPS):
            out = _step(env, b, acts[t], policy)
            recs.append(_rec(site, b, env.get_state()["robot"], out["ob"], out["obs_rotated"], step=t, policy=policy,
                             human_action=np.array(out["human_action"])))
    _close(env)
    return recs


def form_step(make_env, params, b):
    """obs_rotated and ob of STEPS steps with HUMAN_EXTERNAL and with HUMAN_LINEAR (step_kernel)."""
    return _form_step(make_env, params, b, (_abi.HUMAN_EXTERNAL, _abi.HUMAN_LINEAR), "step_kernel")


def form_orca(make_env, params, b):
    """The same with HUMAN_ORCA (the ROWS role of orca_step_kernel)."""
    return _form_step(make_env, params, b, (_abi.HUMAN_ORCA,), "orca_step_kernel")


def form_lookahead(make_env, params, b, A=None, policies=(_abi.HUMAN_EXTERNAL, _abi.HUMAN_LINEAR, _abi.HUMAN_ORCA)):
    """rows_rotated and next_ob of one look-ahead per policy, from reset; the robot state is the propagated one,
    computed here per action.  Under unicycle `exact` marks the frames whose propagation holds no cos / sin but of 0:
    rotation 0 from heading 0."""
    uni = _unicycle(params)
    actions = la_actions(81 if A is None else A, uni)
    env = make_env(params, b.n, b.N, b.S)
    recs = []
    for policy in policies:
        env.reset(b)
        if policy == _abi.HUMAN_EXTERNAL:
            env.set_human_actions(external_actions(b))
        robot = env.get_state()["robot"]
        la = env.lookahead(actions, human_policy=policy)
        r = _rec("lookahead_kernel", b, propagate(robot, actions, uni, params.time_step), la["next_ob"][:, None],
                 la["rows_rotated"], policy=policy, actions=actions)
        r["types"], r["n_rows"] = r["types"][:, None], r["n_rows"][:, None]
        exact = np.ones((b.n, len(actions)), bool)
        if uni:
            exact = (robot[:, None, 8] == 0.0) & (actions[None, :, 1] == 0.0)
        r["exact"] = exact
        recs.append(r)
    _close(env)
    return recs


def form_one_launch(make_env, params, b, K=STEPS):
    """ebc_step_k with FLAG_ONE_LAUNCH, K steps: state_rotated[k] (the rollout kernel's state rows) and obs_rotated[k]
    (its rows of humans and of static rows).  The robot states and the raw rows come from the per-step form run beside
    it on a second env: the two forms hold the same states bit for bit (tests/test_step_k_one_launch_gpu.py)."""
    acts = robot_actions(K, b.n, _unicycle(params))
    env = make_env(params, b.n, b.N, b.S)
    env.reset(b)
    kw = dict(robot_action=acts, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_EXTERNAL)
    one = env.step_k(K, ("state_rotated", "obs_rotated"), flags=_abi.FLAG_ONE_LAUNCH, **kw)
    after = env.get_state()
    _close(env)
    side = make_env(params, b.n, b.N, b.S)
    side.reset(b)
    recs = []
    for k in range(K):
        ob, per_step_state = side.observe()
        recs.append(_rec("rollout_kernel state_rotated", b, side.get_state()["robot"], ob, one["state_rotated"][k], step=k,
                         per_step=per_step_state))
        out = side.step(robot_action=acts[k], human_policy=_abi.HUMAN_ORCA)
        recs.append(_rec("rollout_kernel obs_rotated", b, side.get_state()["robot"], out["ob"], one["obs_rotated"][k],
                         step=k, per_step=np.array(out["obs_rotated"])))
    st = side.get_state()
    for key in ("robot", "px", "py", "vx", "vy"):  # the premise, checked where it is used
        assert st[key].tobytes() == after[key].tobytes(), "one-launch and per-step states differ: " + key
    _close(side)
    return recs


ROW_FORMS = {"observe": form_observe, "step": form_step, "orca": form_orca, "lookahead": form_lookahead,
             "one_launch": form_one_launch}
FORM_SHAPE = (67, 6, 3)  # (E, N, S) of the forms' batches: R = 9 rows; 81 * 9 look-ahead rows are 3 chunks per env
WIDTHS = (13, 17)


def form_batch(form, T, unicycle, E=FORM_SHAPE[0]):
    """The batch a form runs on: under unicycle the look-ahead's robots head exactly 0."""
    import zlib
    rs = np.random.RandomState(zlib.crc32(("%s-%d-%d" % (form, T, unicycle)).encode()) % 2 ** 31)
    return probe_batch(rs, E, FORM_SHAPE[1], FORM_SHAPE[2], theta=0.0 if (unicycle and form == "lookahead") else None)


def run_form(make_env, form, T, unicycle):
    params = rows_params(T, unicycle)
    return params, ROW_FORMS[form](make_env, params, form_batch(form, T, unicycle))


# ---- the look-ahead's shapes ------------------------------------------------------------------------------------------

LA_E = 5
# (A, N, S): R = N + S
LA_SHAPES = [(1, 1, 0), (51, 4, 1), (64, 3, 1), (128, 2, 0), (37, 5, 2), (81, 4, 1), (27, 12, 7), (81, 11, 7),
             (128, 33, 95)]
LA_UNICYCLE = [(81, 4, 1), (37, 5, 2)]
LA_CASES = ([(A, N, S, T, 0) for (A, N, S) in LA_SHAPES for T in WIDTHS]
            + [(A, N, S, T, 1) for (A, N, S) in LA_UNICYCLE for T in WIDTHS])


def la_case_id(case):
    return "A%d-R%d-T%d%s" % (case[0], case[1] + case[2], case[3], "-unicycle" if case[4] else "")


def copy_split(E, A, R, T):
    """The flat 16-byte copy of lookahead_kernel's phase C restated: per env and per chunk of 256 rows
    (head, body, tail, rows): scalar floats before the first 16-byte boundary, float4 stores, scalar floats behind."""
    total = A * R
    out = []
    for e in range(E):
        base = e * total * T
        for c0 in range(0, total, LA_THREADS):
            rows = min(LA_THREADS, total - c0)
            cnt = rows * T
            head = (4 - ((base + c0 * T) & 3)) & 3
            body = (cnt - head) // 4 if cnt > head else 0
            tail = max(cnt - head - 4 * body, 0)
            out.append((min(head, cnt), body, tail, rows))
    return out


def la_batch(case):
    A, N, S, T, uni = case
    rs = np.random.RandomState(9000 + 100 * A + N + S + T + uni)
    return probe_batch(rs, LA_E, N, S, theta=0.0 if uni else None)
